"""cid_search_perfect_segments / cid_search_perfect_segments_dev against the oracle, segment by segment and bit-exact: the AND words of
a segment equal Index.search_perfect on the segment's k-mers alone (zero where the oracle flags an absent row, and for an empty
segment), the flag equals the oracle's, and no bit at or above n_colors is set.

The layouts and the segment lengths are those of test_gpu_segments.py (rows of 1, 2, 4, 8, 16 and 128 words, n_hash 5, one k > 32; empty
segments, 63 / 64 / 65 and 127 / 129 k-mers around the tile, 200 segments of one k-mer, one of 5 000 that spans twenty workgroups).  The
index is a copy of that module's, planted further: the 65-, 300- and 5 000-k-mer segments into one colour as there, and the 200 one-k-mer
segments alternately into two other colours — neighbours inside one tile then have different answers, so an AND that leaks across a segment
boundary shows.  The k-mers of the 63- and 127-k-mer segments go alternately into the same two colours: every row is there and no colour
holds them all, the outcome that is neither a hit nor the flag.  In the layouts whose Bloom filter is small against the planted k-mers nearly every row ends up non-zero, so not every
layout can show every outcome: test_every_outcome_occurs checks the table as a whole, on the same references."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_segments as seg
from test_gpu_segments import LAYOUTS, PLANTED, SEG_LENS
from util import to_hip_index

pytestmark = pytest.mark.gpu

LENS = np.array(SEG_LENS)
NO_COMMON = (63, 127)     # their k-mers go alternately into the two colours of the one-k-mer segments
_cases = {}


def case(orc, layout):
    """(oracle index, k-mers, seg_off, words wanted [n_segs, w32] uint32 — zero where flagged or empty —, flags wanted [n_segs] bool): made once"""
    if layout in _cases:
        return _cases[layout]
    n_colors, n_hash, k, m = layout
    base, kmers, seg_off = seg.case(orc, layout)[:3]          # shared with test_gpu_segments, and left as it is: planted into a copy
    oix = orc.Index(m, n_hash, k, n_colors)
    oix.rows()[:] = base.rows()
    main = n_colors // 2
    two = [c for c in (0, n_colors - 1, 1, 2) if c != main][:2]
    ones = [s for s, n in enumerate(SEG_LENS) if n == 1][-200:]
    assert len(ones) == 200 and ones == list(range(ones[0], ones[0] + 200))
    for j, s in enumerate(ones):
        oix.insert(two[j & 1], kmers[int(seg_off[s])].tobytes())
    for s, n in enumerate(SEG_LENS):          # ... and segments whose rows are all there but share no colour: neither a hit nor the flag
        if n in NO_COMMON:
            for j, km in enumerate(kmers[int(seg_off[s]):int(seg_off[s + 1])]):
                oix.insert(two[j & 1], km.tobytes())
    words = np.zeros((len(SEG_LENS), oix.w32), np.uint32)
    missing = np.zeros(len(SEG_LENS), bool)
    for s, n in enumerate(SEG_LENS):
        if n:
            w, missing[s] = oix.search_perfect(kmers[int(seg_off[s]):int(seg_off[s + 1])])
            words[s] = 0 if missing[s] else w
    for a in (words, missing):
        a.setflags(write=False)
    _cases[layout] = (oix, kmers, seg_off, words, missing, (main, two))
    return _cases[layout]


def outcomes(words, missing):
    perfect = (LENS > 0) & ~missing & words.any(axis=1)
    return perfect, missing, (LENS > 0) & ~missing & ~perfect


def bit(words, c):
    return (words[:, c // 32] >> np.uint32(c % 32)) & np.uint32(1)


def check(layout, got_words, got_missing, want_words, want_missing):
    bad = np.flatnonzero((got_words != want_words).any(axis=1))
    print(f"{layout}: {len(bad)} segments differ in the words, {int((got_missing != want_missing).sum())} in the flag")
    assert len(bad) == 0, f"segments {bad[:10]} (lengths {[SEG_LENS[i] for i in bad[:10]]})"
    assert np.array_equal(got_missing, want_missing)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "C%d-n%d-k%d-m%d" % l)
def test_perfect_segments_match_the_oracle(orc, hip_ctx, layout):
    oix, kmers, seg_off, want_words, want_missing, (main, two) = case(orc, layout)
    n_colors = layout[0]
    hx = to_hip_index(hip_ctx, oix)
    got_words, got_missing = hx.search_perfect_segments(kmers, seg_off)
    assert got_words.shape == want_words.shape and got_words.dtype == np.uint32 and got_missing.dtype == bool
    check(layout, got_words, got_missing, want_words, want_missing)
    # zero where the oracle flags an absent row or the segment is empty; no bit at or above n_colors
    assert not got_words[want_missing].any() and not got_words[LENS == 0].any() and not got_missing[LENS == 0].any()
    bits = np.unpackbits(got_words.view(np.uint8), axis=1, bitorder="little")
    assert not bits[:, n_colors:].any()
    # the planted segments hit their colour; neighbouring one-k-mer segments carry different colours wherever neither is flagged
    for s, n in enumerate(SEG_LENS):
        if n in PLANTED and not want_missing[s]:
            assert bit(got_words[s:s + 1], main)[0] == 1, s
    # what cid_search_segments' counters imply: colour c iff hits == length
    hits, flags = hx.search_segments(kmers, seg_off)
    assert np.array_equal(flags, got_missing)
    for s, n in enumerate(SEG_LENS):
        implied = seg.perfect_bits(hits[s], n) if n and not flags[s] else np.zeros(oix.w32, np.uint32)
        assert np.array_equal(got_words[s], implied), s
    # a NULL flag pointer gives the same words
    w_only, none = hx.search_perfect_segments(kmers, seg_off, want_missing=False)
    assert none is None and np.array_equal(w_only, want_words)
    # one segment over everything == cid_search_perfect
    one_words, one_missing = hx.search_perfect_segments(kmers, np.array([0, len(kmers)], np.uint64))
    pw, pm = hx.search_perfect(kmers)
    assert bool(one_missing[0]) == pm == oix.search_perfect(kmers)[1] and np.array_equal(one_words[0], pw)
    # no segments at all
    w0, m0 = hx.search_perfect_segments(kmers[:0], np.array([0], np.uint64))
    assert w0.shape == (0, oix.w32) and m0.shape == (0,)
    hx.close()


def test_every_outcome_occurs(orc):
    """over the layout table: segments with a perfect hit, flagged segments, segments with neither — all three within one call for the
    layouts whose Bloom filter the planted k-mers cannot fill — and one-k-mer neighbours whose answers differ"""
    seen = np.zeros(3, int)
    for layout in LAYOUTS:
        _, _, _, words, missing, (main, two) = case(orc, layout)
        o = [int(x.sum()) for x in outcomes(words, missing)]
        print(layout, "perfect / missing / neither:", o)
        seen += o
        assert o[0] >= 1
        if layout != (8192, 2, 31, 1_009):       # (1 009 rows: the planted k-mers leave no row empty and every colour everywhere)
            assert all(o)
        if layout in ((4, 4, 27, 750_000), (256, 4, 31, 1 << 20), (40, 3, 45, 30_011)):
            ones = np.flatnonzero(LENS == 1)[-200:]
            ok = ~missing[ones]
            a, b = bit(words[ones], two[0]), bit(words[ones], two[1])
            even, odd = ok & (np.arange(200) % 2 == 0), ok & (np.arange(200) % 2 == 1)
            assert a[even].all() and b[odd].all()                       # each holds its own colour ...
            assert (a[odd] == 0).any() and (b[even] == 0).any()         # ... and not, all of them, the neighbour's
    assert all(seen)


@pytest.mark.parametrize("switches", [("upload_chunk_bytes",), ("dense_report_bytes",), ("upload_chunk_bytes", "dense_report_bytes")], ids=lambda s: "+".join(s))
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2], LAYOUTS[5], LAYOUTS[6]], ids=lambda l: "C%d" % l[0])
def test_chunked_uploads_and_sliced_words_change_nothing(orc, layout, switches):
    """one tile of 64 k-mers per upload chunk — every longer segment is ANDed by several launches into one row, and chunks cut across
    runs of short segments — alone, and with one segment's words per slice of the device copy; and such slices alone"""
    import colorid_amd
    oix, kmers, seg_off, want_words, want_missing, _ = case(orc, layout)
    k = layout[2]
    ctx = colorid_amd.Context(0)
    try:
        hx = to_hip_index(ctx, oix)
        rs = hx.device_matrix()[1]
        for sw in switches:
            ctx.tune(sw, 64 * (k + 8) if sw == "upload_chunk_bytes" else rs * 8)
        got_words, got_missing = hx.search_perfect_segments(kmers, seg_off)
        check(layout, got_words, got_missing, want_words, want_missing)
        assert np.array_equal(hx.search_perfect_segments(kmers, seg_off, want_missing=False)[0], want_words)
        hx.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2], LAYOUTS[3], LAYOUTS[6]], ids=lambda l: "C%d" % l[0])
def test_device_pointer_form(orc, hip_ctx, layout):
    import torch
    oix, kmers, seg_off, want_words, want_missing, _ = case(orc, layout)
    n_segs = len(SEG_LENS)
    hx = to_hip_index(hip_ctx, oix)
    rs = hx.device_matrix()[1]
    host_words, host_missing = hx.search_perfect_segments(kmers, seg_off)
    dk = torch.from_numpy(kmers.reshape(-1).copy()).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    d_words = torch.full((n_segs, rs), 0x5A5A5A5A12345678, dtype=torch.int64, device="cuda")   # neither zero nor all ones: the call presets
    d_miss = torch.full((n_segs,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def words_le():
        w = d_words.cpu().numpy().view("<u4")
        assert not w[:, oix.w32:].any()                       # the row's padding words are zero
        return w[:, :oix.w32]

    hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, len(kmers), d_words.data_ptr(), d_miss.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(words_le(), host_words) and np.array_equal(host_words, want_words)
    assert np.array_equal(d_miss.cpu().numpy().astype(bool), host_missing) and np.array_equal(host_missing, want_missing)
    d_words.fill_(0x0101010101010101)
    torch.cuda.synchronize()
    hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, len(kmers), d_words.data_ptr(), None)   # no flags wanted
    hip_ctx.synchronize()
    assert np.array_equal(words_le(), want_words)
    before = d_words.clone()
    hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), 0, 0, d_words.data_ptr(), None)                 # nothing to do, nothing touched
    hip_ctx.synchronize()
    assert torch.equal(before, d_words)
    hx.close()


def test_errors(orc, hip_ctx):
    import colorid_amd
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    layout = LAYOUTS[1]
    oix, kmers, seg_off, want_words, want_missing, _ = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    lib, vp = hip_ctx.lib, C.c_void_p

    def code(f):
        with pytest.raises(colorid_amd.CidError) as e:
            f()
        return e.value.code

    def good():
        w, f = hx.search_perfect_segments(kmers, seg_off)
        assert np.array_equal(w, want_words) and np.array_equal(f, want_missing)

    def raw(kmers_p, off_p, n_segs, words_p):
        return lib.cid_search_perfect_segments(hip_ctx.h, hx.h, kmers_p, off_p, n_segs, words_p, None)

    words = np.full((3, oix.w32), 0xABCD, np.uint32)
    off = np.array([0, 1, 2, 3], np.uint64)
    assert raw(kmers.ctypes.data_as(vp), off.ctypes.data_as(vp), 3, None) == INVALID           # null words
    assert raw(kmers.ctypes.data_as(vp), None, 3, words.ctypes.data_as(vp)) == INVALID         # null seg_off
    assert raw(None, off.ctypes.data_as(vp), 3, words.ctypes.data_as(vp)) == INVALID           # null k-mers
    assert lib.cid_search_perfect_segments(None, hx.h, kmers.ctypes.data_as(vp), off.ctypes.data_as(vp), 3, words.ctypes.data_as(vp), None) == INVALID
    assert raw(None, None, 0, None) == 0 and (words == 0xABCD).all()                           # no segments: CID_OK, nothing touched
    good()
    assert code(lambda: hx.search_perfect_segments(kmers, np.array([1, 2, 3], np.uint64))) == INVALID         # seg_off[0] != 0
    assert code(lambda: hx.search_perfect_segments(kmers, np.array([0, 5, 3, 9], np.uint64))) == INVALID      # decreasing
    assert code(lambda: hx.search_perfect_segments(kmers, np.array([0, 2, (1 << 32) + 2], np.uint64))) == INVALID   # a segment of 2^32 k-mers
    good()
    fresh = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8)
    assert code(lambda: fresh.search_perfect_segments(kmers[:3], off)) == STATE                                # not finalized
    fresh.close()
    mini = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8).set_minimizer(11).finalize()
    assert code(lambda: mini.search_perfect_segments(kmers[:3], off)) == UNSUPPORTED                           # a minimizer index
    mini.close()
    wide = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8193).finalize()
    assert code(lambda: wide.search_perfect_segments(kmers[:3], off)) == UNSUPPORTED                           # rows of more than 128 words
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert code(lambda: wide.search_perfect_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr())) == UNSUPPORTED
    assert code(lambda: hx.search_perfect_segments_dev(d.data_ptr(), None, 1, 1, d.data_ptr())) == INVALID
    assert code(lambda: hx.search_perfect_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, None)) == INVALID
    wide.close()
    good()
    hx.close()


@pytest.mark.parametrize("layout", seg.WALK_LAYOUTS, ids=lambda l: "C%d" % l[0])
def test_a_wave_with_several_tiles(orc, hip_ctx, layout):
    """test_gpu_segments' launch of two tiles a wave and its references (walk_case): the running AND carried from a wave's first tile to
    its second, flushed between two segments, and flushed before a boundary tile"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cs = seg.walk_case(orc, layout, n_cu)
    seg_off, n_segs, n_kmers = cs["seg_off"], len(cs["seg_off"]) - 1, len(cs["idx"])
    seg.check_walk_covers_the_tile_pairs(seg_off, n_cu)
    oix = cs["oix"]
    hx = to_hip_index(hip_ctx, oix)
    rs = hx.device_matrix()[1]
    dk = torch.from_numpy(cs["pool"][cs["idx"]].reshape(-1)).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    d_words = torch.full((n_segs, rs), 0x5A5A5A5A12345678, dtype=torch.int64, device="cuda")
    d_miss = torch.full((n_segs,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hx.search_perfect_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, n_kmers, d_words.data_ptr(), d_miss.data_ptr())
    hip_ctx.synchronize()
    w = d_words.cpu().numpy().view("<u4")
    assert not w[:, oix.w32:].any()
    got_words, got_missing = w[:, :oix.w32], d_miss.cpu().numpy().astype(bool)
    bad = np.flatnonzero((got_words != cs["words"]).any(axis=1))
    print(f"{layout}: {n_segs} segments, {len(bad)} differ in the words, {int((got_missing != cs['missing']).sum())} in the flag; "
          f"{int(cs['words'].any(axis=1).sum())} with a perfect hit")
    assert len(bad) == 0, f"segments {bad[:10]} (lengths {np.diff(seg_off)[bad[:10]]})"
    assert np.array_equal(got_missing, cs["missing"])
    # the planted classes: a perfect hit in c0 and c1, in c1 alone, in c1 and c2 — neighbours differ
    c0, c1, c2 = cs["colours"]
    lens = np.diff(seg_off)
    for cls, (have, lack) in enumerate((((c0, c1), (c2,)), ((c1,), (c0, c2)), ((c1, c2), (c0,)))):
        s = np.flatnonzero((np.arange(n_segs) % 7 == cls) & (lens >= 28))
        assert len(s) and all(bit(got_words[s], c).all() for c in have) and not any(bit(got_words[s], c).any() for c in lack), cls
    hx.close()
