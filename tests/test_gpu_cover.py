"""cid_search_cover / cid_search_cover_dev against tests/cover_ref.py on the oracle's bits: P[w] is the oracle's perfect search of window
w's k-mer alone (its AND word, unpacked), forced to zero for the invalid windows, and all seven statistics of every (segment, colour)
must be equal.

One call holds every shape of segment around the 64-window tile (0, 1, 63, 64, 65, 127, 129, 300, 1000 windows, empty ones in front, in a
row and at the end, a hundred segments of one window inside two tiles).  Windows 0..99 and 150..299 of the 300-window segment and windows
0..499 and 500+k..999 of the 1000-window one are inserted into colour C // 2: one gap above k - 1 and one of exactly k.  About 3 % of the
windows are invalid and carry b"N" * k as their k-mer; the 129- and 300-window segments repeat a stretch of 20 k-mers later in the
segment, FIRST cleared, so that kmers_hit < windows_hit occurs."""
import numpy as np
import pytest

import cover_ref
from cover_ref import WIN_FIRST, WIN_VALID
from util import random_index, random_kmers, to_hip_index

gpu = pytest.mark.gpu

# (n_colors, n_hash, k, bloom_size)
LAYOUTS = [
    (4, 4, 27, 750_000),        # rs = 1
    (129, 4, 31, 40_009),       # dead lanes, rs = 4
    (1024, 2, 31, 10_007),
    (8192, 2, 31, 1_009),
    (40, 3, 45, 30_011),        # k > 32
]
SEG_LENS = [0, 1, 63, 64, 65, 0, 0, 127, 129, 300, 1] + [1] * 100 + [1000, 0]
S129, S300, S1000 = SEG_LENS.index(129), SEG_LENS.index(300), SEG_LENS.index(1000)
REPEATS = {S129: (10, 100), S300: (160, 250)}     # segment -> (source, copy) of a stretch of 20 k-mers
UNSUPPORTED = -4
ids = lambda l: "C%d-n%d-k%d-m%d" % l

_cases = {}


def case(orc, layout):
    """(oracle index, k-mers, seg_off, flags, wanted cells [n_segs, C]): made once per layout and left unchanged"""
    if layout in _cases:
        return _cases[layout]
    n_colors, n_hash, k, m = layout
    rng = np.random.default_rng(n_colors * 977 + k)
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.3, zero_row_frac=0.15)
    seg_off = np.zeros(len(SEG_LENS) + 1, np.uint64)
    seg_off[1:] = np.cumsum(SEG_LENS)
    off = [int(x) for x in seg_off]
    W = off[-1]
    kmers = random_kmers(rng, W, k)
    valid = rng.random(W) >= 0.03
    for s, (src, dst) in REPEATS.items():
        kmers[off[s] + dst:off[s] + dst + 20] = kmers[off[s] + src:off[s] + src + 20]
        valid[off[s] + src:off[s] + src + 20] = valid[off[s] + dst:off[s] + dst + 20] = True
    planted = [(S300, 0, 100), (S300, 150, 300), (S1000, 0, 500), (S1000, 500 + k, 1000)]
    for s, a, b in planted:
        for w in range(off[s] + a, off[s] + b):
            if valid[w]:
                oix.insert(n_colors // 2, kmers[w].tobytes())
    kmers[~valid] = ord("N")                                     # garbage that must not be hashed
    flags = np.zeros(W, np.uint8)
    flags[valid] = WIN_VALID
    for s in range(len(SEG_LENS)):
        seen = set()
        for w in range(off[s], off[s + 1]):
            if valid[w] and kmers[w].tobytes() not in seen:
                seen.add(kmers[w].tobytes())
                flags[w] |= WIN_FIRST
    P = np.zeros((W, n_colors), bool)
    for w in np.flatnonzero(valid):
        words = oix.search_perfect(kmers[w:w + 1])[0]
        P[w] = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_colors]
    want = np.zeros((len(SEG_LENS), n_colors), cover_ref.DTYPE)
    for s in range(len(SEG_LENS)):
        want[s] = cover_ref.cover(P[off[s]:off[s + 1]], (flags[off[s]:off[s + 1]] & WIN_FIRST) != 0, k)
    for a in (kmers, seg_off, flags, want):
        a.setflags(write=False)
    _cases[layout] = (oix, kmers, seg_off, flags, want)
    return _cases[layout]


def assert_cells_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == cover_ref.DTYPE
    for f in cover_ref.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, f"{what}{f}: {len(bad)} cells differ, first (segment, colour) {bad[:5].tolist()} " \
                              f"(lengths {[SEG_LENS[s] for s, _ in bad[:5]]}): got {got[f][tuple(bad[0])]}, want {want[f][tuple(bad[0])]}"
    assert not got["reserved"].any()


def test_the_table_shows_every_outcome(orc):
    """on the REFERENCE values, so that a sparse index cannot make the comparison vacuous: cells with three runs or more, cells whose runs
    merge (bases_covered below windows_hit + n_runs * (k - 1)), cells that start after window 0, cells with kmers_hit < windows_hit;
    and the planted colour shows the two planted gaps"""
    seen = np.zeros(4, int)
    for layout in LAYOUTS:
        n_colors, _, k, _ = layout
        _, _, _, flags, want = case(orc, layout)
        w = want
        hit = w["windows_hit"] > 0
        o = [int((w["n_runs"] >= 3).sum()), int((hit & (w["bases_covered"] < w["windows_hit"] + w["n_runs"] * (k - 1))).sum()),
             int((hit & (w["first_window"] > 0)).sum()), int((w["kmers_hit"] < w["windows_hit"]).sum())]
        print(layout, "cells with >= 3 runs / merged gaps / first_window > 0 / kmers_hit < windows_hit:", o, "invalid windows:",
              int((flags & WIN_VALID == 0).sum()))
        seen += o
        if n_colors >= 129:     # 0.3 ^ n_hash of the cells' windows hit by chance
            assert all(o)
        c300, c1000 = w[S300, n_colors // 2], w[S1000, n_colors // 2]
        assert c300["windows_hit"] >= 225 and c300["kmers_hit"] < c300["windows_hit"] and c1000["windows_hit"] >= 900   # 250 and 1000 - k planted, ~3 % invalid
    assert all(seen)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_cover_matches_the_reference(orc, hip_ctx, layout):
    oix, kmers, seg_off, flags, want = case(orc, layout)
    n_colors = layout[0]
    hx = to_hip_index(hip_ctx, oix)
    got = hx.search_cover(kmers, seg_off, flags)
    assert_cells_equal(got, want)
    empty = np.array(SEG_LENS) == 0
    assert not got["windows_hit"][empty].any() and (got["first_window"][empty] == cover_ref.NONE).all() and (got["last_window"][empty] == cover_ref.NONE).all()
    # kmers_hit is the segmented search on the FIRST windows alone
    first = (flags & (WIN_VALID | WIN_FIRST)) == (WIN_VALID | WIN_FIRST)
    off_first = np.concatenate(([0], np.cumsum(first)))[seg_off.astype(np.int64)].astype(np.uint64)
    hits, _ = hx.search_segments(kmers[first], off_first, want_missing=False)
    assert np.array_equal(hits, got["kmers_hit"])
    # no flags == every window VALID and FIRST (on k-mers that can be hashed)
    clean = np.where((flags & WIN_VALID)[:, None] != 0, kmers, np.uint8(ord("A")))
    no_flags = hx.search_cover(clean, seg_off, None)
    assert_cells_equal(no_flags, hx.search_cover(clean, seg_off, np.full(len(clean), WIN_VALID | WIN_FIRST, np.uint8)), "flags=None: ")
    assert np.array_equal(no_flags["kmers_hit"], no_flags["windows_hit"])
    # no segments at all; empty segments alone
    assert hx.search_cover(kmers[:0], np.array([0], np.uint64)).shape == (0, n_colors)
    none = hx.search_cover(kmers[:0], np.array([0, 0, 0], np.uint64))
    assert_cells_equal(none, want[[0, 5]])
    hx.close()


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_device_pointer_form(orc, hip_ctx, layout):
    import torch
    oix, kmers, seg_off, flags, want = case(orc, layout)
    n_colors, n_segs = layout[0], len(SEG_LENS)
    hx = to_hip_index(hip_ctx, oix)
    dk = torch.from_numpy(kmers.reshape(-1).copy()).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    df = torch.from_numpy(flags.copy()).cuda()
    d_out = torch.full((n_segs, n_colors, 8), -559038737, dtype=torch.int32, device="cuda")   # garbage: every cell is written
    torch.cuda.synchronize()
    hx.search_cover_dev(dk.data_ptr(), do.data_ptr(), df.data_ptr(), n_segs, len(kmers), d_out.data_ptr())
    hip_ctx.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(n_segs, n_colors * 8).view(cover_ref.DTYPE)
    assert_cells_equal(got, want, "_dev: ")
    assert_cells_equal(got, hx.search_cover(kmers, seg_off, flags), "_dev against the host form: ")
    hx.search_cover_dev(dk.data_ptr(), do.data_ptr(), df.data_ptr(), 0, 0, d_out.data_ptr())   # nothing to do
    hip_ctx.synchronize()
    hx.close()


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_slices_change_nothing_and_a_segment_that_cannot_fit_is_refused(orc, layout):
    """dense_report_bytes = what the 1000-window segment needs (its scratch rows and its output cells) and two more segments' cells: the
    call takes many slices, cut at whole segments; with 64-window upload chunks a slice's k-mers go up in pieces as well.  One byte
    less than the largest segment needs: CID_ERR_UNSUPPORTED."""
    import colorid_amd
    oix, kmers, seg_off, flags, want = case(orc, layout)
    n_colors, _, k, _ = layout
    ctx = colorid_amd.Context(0)
    try:
        hx = to_hip_index(ctx, oix)
        rs = hx.device_matrix()[1]
        need = 1000 * rs * 8 + n_colors * 32
        ctx.tune("dense_report_bytes", need + 2 * n_colors * 32)
        assert_cells_equal(hx.search_cover(kmers, seg_off, flags), want, "sliced: ")
        ctx.tune("upload_chunk_bytes", 64 * (k + 8))
        assert_cells_equal(hx.search_cover(kmers, seg_off, flags), want, "sliced, chunked uploads: ")
        ctx.tune("dense_report_bytes", need)
        assert_cells_equal(hx.search_cover(kmers, seg_off, flags), want, "exact fit: ")
        ctx.tune("dense_report_bytes", need - 1)
        with pytest.raises(colorid_amd.CidError) as e:
            hx.search_cover(kmers, seg_off, flags)
        assert e.value.code == UNSUPPORTED and "dense_report_bytes" in str(e.value)
        ctx.tune("dense_report_bytes", 1 << 31)
        ctx.tune("upload_chunk_bytes", 64 * (k + 8))
        assert_cells_equal(hx.search_cover(kmers, seg_off, flags), want, "one slice, chunked uploads: ")
    finally:
        ctx.close()


@gpu
def test_errors(orc, hip_ctx):
    import ctypes as C

    import colorid_amd
    INVALID, STATE = -1, -5
    layout = LAYOUTS[1]
    oix, kmers, seg_off, flags, want = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    lib, vp = hip_ctx.lib, C.c_void_p

    def code(f):
        with pytest.raises(colorid_amd.CidError) as e:
            f()
        return e.value.code

    out = np.zeros((3, layout[0]), cover_ref.DTYPE)
    off = np.array([0, 1, 2, 3], np.uint64)
    p = lambda a: a.ctypes.data_as(vp)
    assert lib.cid_search_cover(hip_ctx.h, hx.h, p(kmers), p(off), None, 3, None) == INVALID          # null out
    assert lib.cid_search_cover(hip_ctx.h, hx.h, p(kmers), None, None, 3, p(out)) == INVALID          # null seg_off
    assert lib.cid_search_cover(hip_ctx.h, hx.h, None, p(off), None, 3, p(out)) == INVALID            # null k-mers
    assert lib.cid_search_cover(None, hx.h, p(kmers), p(off), None, 3, p(out)) == INVALID
    assert code(lambda: hx.search_cover(kmers, np.array([1, 2, 3], np.uint64))) == INVALID            # seg_off[0] != 0
    assert code(lambda: hx.search_cover(kmers, np.array([0, 5, 3, 9], np.uint64))) == INVALID         # decreasing
    fresh = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8)
    assert code(lambda: fresh.search_cover(kmers[:3], off)) == STATE                                  # not finalized
    fresh.close()
    mini = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8).set_minimizer(11).finalize()
    assert code(lambda: mini.search_cover(kmers[:3], off)) == UNSUPPORTED                             # a minimizer index
    mini.close()
    wide = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8193).finalize()
    assert code(lambda: wide.search_cover(kmers[:3], off)) == UNSUPPORTED                             # more than 8192 colours
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert code(lambda: wide.search_cover_dev(d.data_ptr(), d.data_ptr(), None, 1, 1, d.data_ptr())) == UNSUPPORTED
    assert code(lambda: hx.search_cover_dev(d.data_ptr(), None, None, 1, 1, d.data_ptr())) == INVALID
    wide.close()
    assert_cells_equal(hx.search_cover(kmers, seg_off, flags), want, "after the refusals: ")
    hx.close()
