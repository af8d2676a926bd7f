"""cid_search_nearest_segments / cid_search_nearest_segments_dev against a reference over the oracle's per-segment counters, all four
fields of every cell bit-exact.

The definition (include/colorid_hip.h).  hits[s][c] = cid_search_segments' counter, len_s = the segment's k-mer count.  For group g and
colour c the candidates are the segments s of g with len_s > 0 and hits[s][c] > 0, ordered by share hits / len descending — compared
exactly as hits_a * len_b against hits_b * len_a — with ties to the lowest s.  The cell is {seg = the best s, kmers_hit, n_kmers = its
length, n_perfect = the segments of g with len_s > 0 and hits == len_s}, or {NEAREST_NONE, 0, 0, 0} without a candidate.  reference()
is that text in Python integers, walking the segments in order.

First case: the layouts and segment lengths of test_gpu_segments.py, whose case() gives the oracle's counters, cut into GROUP_OFF: leading
and trailing empty groups, an empty group between others, a group of empty segments only, one-segment groups, a group over the 63 / 64 /
65-k-mer segments around the tile, and one group of the 200 one-k-mer segments with the 5 000-k-mer one (shares of exactly 1 and 0 two
hundred times over: the lowest segment has to win).  Second case, on the 65- and the 256-colour layout: 3 000 segments of 1 to 3 k-mers,
among them planted pairs A = (x, y), B = (x, y', x', y'') with x and x' inserted into one colour — shares 1/2 and 2/4 — as ONE group, as
3 000 groups, and cut at random into groups of 0 to 12."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_segments as seg
from test_gpu_segments import LAYOUTS, SEG_LENS
from util import random_index, random_kmers, to_hip_index

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
LENS = np.array(SEG_LENS)
#            empty, empty | seg 0 (no k-mers) | 1 | 63 64 65 | empty | two empty segments | 127 | 129 | 300 | 1 x 201 and 5 000 | the last, empty | empty, empty
GROUP_OFF = np.array([0, 0, 0, 1, 2, 5, 5, 7, 8, 9, 10, 212, 213, 213, 213], np.uint64)
assert len(SEG_LENS) == 213 and list(LENS[2:5]) == [63, 64, 65] and not LENS[5:7].any() and set(LENS[10:211]) == {1} and LENS[211] == 5000


def reference(hits, lens, group_off):
    """-> (cells [n_groups, C] of NEAREST_DTYPE, ties [n_groups, C]: candidates that equal the winner's share without being it,
    odd_ties: the same where the share is below 1 and the lengths differ)"""
    from colorid_amd.hip import NEAREST_DTYPE
    n_groups, n_colors = len(group_off) - 1, hits.shape[1]
    out = np.zeros((n_groups, n_colors), NEAREST_DTYPE)
    ties = np.zeros((n_groups, n_colors), np.int64)
    odd_ties = np.zeros((n_groups, n_colors), np.int64)
    for g in range(n_groups):
        b_seg = np.full(n_colors, NONE, object)
        b_hit, b_len, n_perfect = np.zeros(n_colors, object), np.zeros(n_colors, object), np.zeros(n_colors, object)
        for s in range(int(group_off[g]), int(group_off[g + 1])):
            ln = int(lens[s])
            if ln == 0:
                continue
            h = hits[s].astype(object)                                   # Python integers from here on
            cand = (h > 0).astype(bool)
            first = cand & (b_seg == NONE).astype(bool)
            better = cand & ~first & (h * b_len > b_hit * ln).astype(bool)
            equal = cand & ~first & (h * b_len == b_hit * ln).astype(bool)
            take = first | better
            ties[g][take] = 0
            odd_ties[g][take] = 0
            ties[g][equal] += 1
            odd_ties[g][equal & (h < ln).astype(bool) & (b_len != ln).astype(bool)] += 1
            b_seg[take], b_hit[take], b_len[take] = s, h[take], ln
            n_perfect += (h == ln).astype(int)
        out[g]["seg"], out[g]["kmers_hit"], out[g]["n_kmers"], out[g]["n_perfect"] = b_seg, b_hit, b_len, n_perfect
    return out, ties, odd_ties


_refs = {}


def first_case(orc, layout):
    if layout not in _refs:
        oix, kmers, seg_off, hits, _, _ = seg.case(orc, layout)
        _refs[layout] = (oix, kmers, seg_off, hits) + reference(hits, LENS, GROUP_OFF)
    return _refs[layout]


def same(got, want):
    for f in ("seg", "kmers_hit", "n_kmers", "n_perfect"):
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, f"{f}: {len(bad)} cells differ, first (group, colour) {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def dev_form(hip_ctx, hx, kmers, seg_off, group_off, n_colors):
    import torch
    from colorid_amd.hip import NEAREST_DTYPE
    n_groups = len(group_off) - 1
    dk = torch.from_numpy(kmers.reshape(-1).copy()).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    dg = torch.from_numpy(group_off.astype(np.int64)).cuda()
    d_out = torch.full((max(n_groups, 1) * n_colors, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")   # garbage: the call presets
    torch.cuda.synchronize()
    hx.search_nearest_segments_dev(dk.data_ptr(), do.data_ptr(), len(seg_off) - 1, len(kmers), dg.data_ptr(), n_groups, d_out.data_ptr())
    hip_ctx.synchronize()
    return d_out.cpu().numpy().view(np.uint32)[:n_groups * n_colors].copy().view(NEAREST_DTYPE).reshape(n_groups, n_colors)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "C%d-n%d-k%d-m%d" % l)
def test_nearest_matches_the_reference(orc, hip_ctx, layout):
    oix, kmers, seg_off, hits, want, _, _ = first_case(orc, layout)
    n_colors = layout[0]
    hx = to_hip_index(hip_ctx, oix)
    got = hx.search_nearest_segments(kmers, seg_off, GROUP_OFF)
    assert got.shape == want.shape
    same(got, want)
    same(dev_form(hip_ctx, hx, kmers, seg_off, GROUP_OFF, n_colors), want)
    # seg lies inside its group; the winner's fields are the segment's
    lo, hi = GROUP_OFF[:-1, None].astype(np.int64), GROUP_OFF[1:, None].astype(np.int64)
    some = got["seg"] != NONE
    s64 = got["seg"].astype(np.int64)
    assert ((s64 >= lo) & (s64 < hi))[some].all()
    assert not got["kmers_hit"][~some].any() and not got["n_kmers"][~some].any() and not got["n_perfect"][~some].any()
    # n_perfect > 0 exactly where some segment of the group has the colour's bit in the segmented perfect search's words
    words, _ = hx.search_perfect_segments(kmers, seg_off)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n_colors]
    for g in range(len(GROUP_OFF) - 1):
        any_bit = bits[int(GROUP_OFF[g]):int(GROUP_OFF[g + 1])].any(axis=0) if GROUP_OFF[g + 1] > GROUP_OFF[g] else np.zeros(n_colors, bool)
        assert np.array_equal(got["n_perfect"][g] > 0, any_bit), g
    # one group over everything, and every segment a group of its own: the segment itself wherever it hits
    all_in_one = np.array([0, len(SEG_LENS)], np.uint64)
    same(hx.search_nearest_segments(kmers, seg_off, all_in_one), reference(hits, LENS, all_in_one)[0])
    each = hx.search_nearest_segments(kmers, seg_off, np.arange(len(SEG_LENS) + 1, dtype=np.uint64))
    hit = (hits > 0) & (LENS[:, None] > 0)
    assert np.array_equal(each["seg"], np.where(hit, np.arange(len(SEG_LENS))[:, None], NONE).astype(np.uint32))
    assert np.array_equal(each["kmers_hit"], np.where(hit, hits, 0)) and np.array_equal(each["n_perfect"], (hit & (hits == LENS[:, None])).astype(np.uint32))
    hx.close()


def test_every_outcome_occurs(orc):
    """on the reference, over the layout table: cells without a candidate, cells with a perfect segment, cells whose best segment is
    imperfect, and cells where several segments share the best share and the lowest index decides"""
    seen = np.zeros(4, int)
    for layout in LAYOUTS:
        want, ties = first_case(orc, layout)[4:6]
        some = want["seg"] != NONE
        o = [int((~some).sum()), int((want["n_perfect"] > 0).sum()), int((some & (want["kmers_hit"] < want["n_kmers"])).sum()), int((ties > 0).sum())]
        print(layout, "none / perfect / imperfect best / tie by index:", o)
        assert o[0] >= 5 * layout[0]         # the empty groups and the groups of empty segments
        assert o[1] >= 1                     # the planted segments
        if layout != LAYOUTS[0]:             # (4 colours in 750 000 rows: a one-k-mer segment hits a colour once in 250 times)
            assert o[3] >= 1                 # the group of one-k-mer segments
        assert ((want["n_perfect"] > 0) <= (want["kmers_hit"] == want["n_kmers"])).all()    # a perfect segment: the best share is 1
        seen += o
    assert all(seen)
    big = first_case(orc, (256, 4, 31, 1 << 20))
    assert (big[4]["seg"][10] != NONE).any() and (big[5][10] > 0).any()       # group 10: the one-k-mer segments and the 5 000-k-mer one


# ---------------------------------------------------------------------------------------------- many short segments

SHORT_LAYOUTS = [LAYOUTS[1], LAYOUTS[3]]     # 65 and 256 colours
N_SHORT, N_PAIRS = 3000, 40
_short = {}


def short_case(orc, layout):
    """(oracle index, k-mers, seg_off, lens, hits [3 000, C], {name: (group_off, reference cells, ties, odd ties)}): made once"""
    if layout in _short:
        return _short[layout]
    n_colors, n_hash, k, m = layout
    rng = np.random.default_rng(n_colors + 7)
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.3, zero_row_frac=0.15)
    lens = rng.integers(1, 4, N_SHORT)
    pairs = rng.choice(np.arange(0, N_SHORT - 1, 2), N_PAIRS, replace=False)      # A at an even index, B right after it
    lens[pairs], lens[pairs + 1] = 2, 4
    seg_off = np.zeros(N_SHORT + 1, np.uint64)
    seg_off[1:] = np.cumsum(lens)
    kmers = random_kmers(rng, int(seg_off[-1]), k)
    colour = n_colors // 3
    for a in pairs:
        ia, ib = int(seg_off[a]), int(seg_off[a + 1])
        kmers[ib] = kmers[ia]                                    # B starts with A's x ...
        for km in (kmers[ia], kmers[ib + 2]):                    # ... and x, x' are in the colour: 1/2 against 2/4 unless a y hits by chance
            oix.insert(colour, km.tobytes())
    hits = np.zeros((N_SHORT, n_colors), np.uint32)
    for s in range(N_SHORT):
        hits[s] = oix.search_count(kmers[int(seg_off[s]):int(seg_off[s + 1])], None, want_unique=False)[0]
    cuts = np.sort(rng.integers(0, N_SHORT + 1, N_SHORT // 6))
    groupings = {"one": np.array([0, N_SHORT], np.uint64), "each": np.arange(N_SHORT + 1, dtype=np.uint64),
                 "random": np.concatenate([[0], cuts, [N_SHORT]]).astype(np.uint64)}
    _short[layout] = (oix, kmers, seg_off, lens, hits, {name: (go,) + reference(hits, lens, go) for name, go in groupings.items()})
    return _short[layout]


@pytest.mark.parametrize("layout", SHORT_LAYOUTS, ids=lambda l: "C%d" % l[0])
def test_many_short_segments_in_one_group_in_their_own_and_cut_at_random(orc, hip_ctx, layout):
    oix, kmers, seg_off, lens, hits, groupings = short_case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    got_hits, _ = hx.search_segments(kmers, seg_off)
    assert np.array_equal(got_hits, hits)
    for name, (go, want, ties, odd_ties) in groupings.items():
        same(hx.search_nearest_segments(kmers, seg_off, go), want)
        same(dev_form(hip_ctx, hx, kmers, seg_off, go, layout[0]), want)
    # what the case was made for, on the reference: one group has ties nearly everywhere; the random groups hold pairs whose equal
    # shares below 1 come from different lengths (1/2 and 2/4), and empty groups
    assert (groupings["one"][2] > 0).mean() > 0.5 and not groupings["each"][2].any()
    go, want, ties, odd_ties = groupings["random"]
    assert (odd_ties > 0).sum() >= 5 and (np.diff(go.astype(np.int64)) == 0).sum() >= 5
    assert (want["seg"] == NONE).any() and (want["n_perfect"] > 0).any() and ((want["seg"] != NONE) & (want["kmers_hit"] < want["n_kmers"])).any()
    hx.close()


# ---------------------------------------------------------------------------------------------- slices and chunks

@pytest.mark.parametrize("switches", [("upload_chunk_bytes",), ("dense_report_bytes",), ("upload_chunk_bytes", "dense_report_bytes")], ids=lambda s: "+".join(s))
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2], LAYOUTS[5]], ids=lambda l: "C%d" % l[0])
def test_slices_and_chunks_that_cut_groups_and_segments_change_nothing(orc, hip_ctx, layout, switches):
    """one tile of 64 k-mers per upload chunk, seven segments' counters per slice: the group of 202 segments is merged over 29 launches,
    the 5 000-k-mer segment counted by 79; the cells equal those of the untuned call"""
    import colorid_amd
    oix, kmers, seg_off, hits, want, _, _ = first_case(orc, layout)
    n_colors, _, k, _ = layout
    hx0 = to_hip_index(hip_ctx, oix)
    untuned = hx0.search_nearest_segments(kmers, seg_off, GROUP_OFF)
    hx0.close()
    ctx = colorid_amd.Context(0)
    try:
        for sw in switches:
            ctx.tune(sw, 64 * (k + 8) if sw == "upload_chunk_bytes" else 7 * n_colors * 4)
        hx = to_hip_index(ctx, oix)
        got = hx.search_nearest_segments(kmers, seg_off, GROUP_OFF)
        same(got, untuned)
        same(got, want)
        hx.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", SHORT_LAYOUTS, ids=lambda l: "C%d" % l[0])
def test_one_segment_per_slice(orc, layout):
    """dense_report_bytes below one row of counters: a launch per segment, 3 000 merges into the one group's cells"""
    import colorid_amd
    oix, kmers, seg_off, lens, hits, groupings = short_case(orc, layout)
    ctx = colorid_amd.Context(0)
    try:
        ctx.tune("dense_report_bytes", 1)
        hx = to_hip_index(ctx, oix)
        for name in ("one", "random"):
            same(hx.search_nearest_segments(kmers[:int(seg_off[400])], seg_off[:401], np.minimum(groupings[name][0], 400)),
                 reference(hits[:400], lens[:400], np.minimum(groupings[name][0], 400))[0])
        hx.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- errors

def test_errors(orc, hip_ctx):
    import colorid_amd
    import torch
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    layout = LAYOUTS[1]
    oix, kmers, seg_off, hits, want, _, _ = first_case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    lib, vp = hip_ctx.lib, C.c_void_p
    n_segs, n_groups = len(SEG_LENS), len(GROUP_OFF) - 1

    def code(f):
        with pytest.raises(colorid_amd.CidError) as e:
            f()
        return e.value.code

    def good():
        same(hx.search_nearest_segments(kmers, seg_off, GROUP_OFF), want)

    def with_groups(*go):
        return code(lambda: hx.search_nearest_segments(kmers, seg_off, np.array(go, np.uint64)))

    out = np.full((n_groups, layout[0], 4), 0xABCD, np.uint32)
    p = lambda a: a.ctypes.data_as(vp)

    def raw(ctx_h, kmers_p, off_p, groups_p, out_p, ns=n_segs, ng=n_groups):
        return lib.cid_search_nearest_segments(ctx_h, hx.h, kmers_p, off_p, ns, groups_p, ng, out_p)

    assert raw(hip_ctx.h, p(kmers), p(seg_off), p(GROUP_OFF), None) == INVALID          # null out
    assert raw(hip_ctx.h, p(kmers), p(seg_off), None, p(out)) == INVALID                # null group_off
    assert raw(hip_ctx.h, p(kmers), None, p(GROUP_OFF), p(out)) == INVALID              # null seg_off
    assert raw(hip_ctx.h, None, p(seg_off), p(GROUP_OFF), p(out)) == INVALID            # null k-mers
    assert raw(None, p(kmers), p(seg_off), p(GROUP_OFF), p(out)) == INVALID             # null context
    assert raw(hip_ctx.h, None, None, None, None, ng=0) == 0 and raw(hip_ctx.h, None, None, None, None, ns=0) == 0   # nothing to do: CID_OK
    assert (out == 0xABCD).all()
    good()
    assert with_groups(1, 5, n_segs) == INVALID                     # group_off[0] != 0
    assert with_groups(0, 9, 5, n_segs) == INVALID                  # descending
    assert with_groups(0, 5, n_segs - 1) == INVALID                 # does not end at n_segs
    assert with_groups(0, 5, n_segs + 1) == INVALID
    assert code(lambda: hx.search_nearest_segments(kmers, np.array([1, 2, 3], np.uint64), np.array([0, 2], np.uint64))) == INVALID       # seg_off[0] != 0
    assert code(lambda: hx.search_nearest_segments(kmers, np.array([0, 5, 3, 9], np.uint64), np.array([0, 3], np.uint64))) == INVALID    # decreasing
    good()
    empty = hx.search_nearest_segments(kmers, seg_off, np.array([0], np.uint64))       # n_groups == 0
    assert empty.shape == (0, layout[0])
    off = np.array([0, 1, 2, 3], np.uint64)
    go = np.array([0, 3], np.uint64)
    fresh = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8)
    assert code(lambda: fresh.search_nearest_segments(kmers[:3], off, go)) == STATE            # not finalized
    fresh.close()
    mini = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8).set_minimizer(11).finalize()
    assert code(lambda: mini.search_nearest_segments(kmers[:3], off, go)) == UNSUPPORTED       # a minimizer index
    mini.close()
    wide = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8193).finalize()
    assert code(lambda: wide.search_nearest_segments(kmers[:3], off, go)) == UNSUPPORTED       # more than 8192 colours
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert code(lambda: wide.search_nearest_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), 1, d.data_ptr())) == UNSUPPORTED
    wide.close()
    assert code(lambda: hx.search_nearest_segments_dev(d.data_ptr(), None, 1, 1, d.data_ptr(), 1, d.data_ptr())) == INVALID
    assert code(lambda: hx.search_nearest_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, None, 1, d.data_ptr())) == INVALID
    assert code(lambda: hx.search_nearest_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), 1, None)) == INVALID
    assert code(lambda: hx.search_nearest_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), 1, d.data_ptr() + 4)) == INVALID   # alignment
    good()
    hx.close()
