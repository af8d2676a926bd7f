"""cid_search_segments / cid_search_segments_dev against the oracle, segment by segment and bit-exact: the row of counters of a
segment equals Index.search_count on the segment's k-mers alone, its flag equals Index.search_perfect's, and colour c is a perfect
hit of the segment exactly when hits[s][c] equals the segment's length (the AND word of the perfect search).

One call holds every shape of segment: empty ones (leading, in a row, trailing), 1, 63 / 64 / 65 and 127 / 129 k-mers around the
64-k-mer tile, 200 segments of one k-mer (far more than 64 segments inside one tile), and one of 5 000 k-mers, which with the minimum of
4 tiles per workgroup spans twenty workgroups.  The k-mers of the 65-, 300- and 5 000-k-mer segments are inserted into one colour first,
so those segments have a perfect hit; random k-mers meet absent rows (zero_row_frac) and give the flag.  In the layouts whose Bloom
filter is small against the 5 365 planted k-mers (10 007 and 1 009 rows) nearly every row carries the planted colour afterwards, so
not every layout can show every outcome: test_every_outcome_occurs checks the table as a whole, on the same references."""
import ctypes as C

import numpy as np
import pytest

from util import random_index, random_kmers, to_hip_index

pytestmark = pytest.mark.gpu

# (n_colors, n_hash, k, bloom_size)
LAYOUTS = [
    (4, 4, 27, 750_000),        # rs = 1
    (65, 2, 21, 50_021),
    (129, 4, 31, 40_009),       # dead lanes
    (256, 4, 31, 1 << 20),
    (300, 5, 31, 20_011),       # n_hash > 4
    (1024, 4, 31, 10_007),
    (8192, 2, 31, 1_009),
    (40, 3, 45, 30_011),        # one k > 32
]
SEG_LENS = [0, 1, 63, 64, 65, 0, 0, 127, 129, 300, 1] + [1] * 200 + [5000] + [0]
PLANTED = (65, 300, 5000)

_cases = {}


def case(orc, layout):
    """(oracle index, k-mers, seg_off, hits wanted [n_segs, C] uint32, flags wanted [n_segs] bool, AND words per segment): made once"""
    if layout in _cases:
        return _cases[layout]
    n_colors, n_hash, k, m = layout
    rng = np.random.default_rng(n_colors * 131 + n_hash)
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.3, zero_row_frac=0.15)
    seg_off = np.zeros(len(SEG_LENS) + 1, np.uint64)
    seg_off[1:] = np.cumsum(SEG_LENS)
    kmers = random_kmers(rng, int(seg_off[-1]), k)
    colour = n_colors // 2
    for s, n in enumerate(SEG_LENS):
        if n in PLANTED:
            for km in kmers[int(seg_off[s]):int(seg_off[s + 1])]:
                oix.insert(colour, km.tobytes())
    hits = np.zeros((len(SEG_LENS), n_colors), np.uint32)
    missing = np.zeros(len(SEG_LENS), bool)
    words = [None] * len(SEG_LENS)
    for s, n in enumerate(SEG_LENS):
        if n == 0:
            continue
        seg = kmers[int(seg_off[s]):int(seg_off[s + 1])]
        hits[s] = oix.search_count(seg, None, want_unique=False)[0]
        words[s], missing[s] = oix.search_perfect(seg)
    for a in (kmers, seg_off, hits, missing):
        a.setflags(write=False)
    _cases[layout] = (oix, kmers, seg_off, hits, missing, words)
    return _cases[layout]


def perfect_bits(hits_row, n):
    """the AND word the counters imply: colour c iff all n k-mers hit it"""
    bits = np.zeros((len(hits_row) + 31) // 32 * 32, np.uint8)
    bits[:len(hits_row)] = (hits_row == n) if n else 0
    return np.packbits(bits, bitorder="little").view("<u4")


def outcomes(hits, missing):
    lens = np.array(SEG_LENS)
    perfect = (lens > 0) & ~missing & (hits == lens[:, None]).any(axis=1)
    return perfect, missing, (lens > 0) & ~missing & ~perfect


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "C%d-n%d-k%d-m%d" % l)
def test_segments_match_the_oracle(orc, hip_ctx, layout):
    oix, kmers, seg_off, want_hits, want_missing, want_words = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    got_hits, got_missing = hx.search_segments(kmers, seg_off)
    bad = np.flatnonzero((got_hits != want_hits).any(axis=1))
    print(f"{layout}: {len(bad)} segments differ in hits, {int((got_missing != want_missing).sum())} in the flag")
    assert len(bad) == 0, f"segments {bad[:10]} (lengths {[SEG_LENS[i] for i in bad[:10]]})"
    assert np.array_equal(got_missing, want_missing)
    # the perfect search's AND word from the counters (cid_search_perfect zeroes it when a row is absent)
    for s, n in enumerate(SEG_LENS):
        if n and not want_missing[s]:
            assert np.array_equal(perfect_bits(got_hits[s], n), want_words[s]), s
    perfect, _, _ = outcomes(got_hits, got_missing)
    assert perfect.any()                                        # the planted segments
    assert not got_hits[np.array(SEG_LENS) == 0].any() and not got_missing[np.array(SEG_LENS) == 0].any()
    # a NULL flag pointer gives the same hits
    assert np.array_equal(hx.search_segments(kmers, seg_off, want_missing=False)[0], want_hits)
    # one segment == cid_search_count
    one_hits, one_missing = hx.search_segments(kmers, np.array([0, len(kmers)], np.uint64))
    assert np.array_equal(one_hits[0].astype(np.uint64), hx.search_count(kmers, None, want_unique=False, want_unique_colour=False)[0])
    assert bool(one_missing[0]) == oix.search_perfect(kmers)[1]
    # no segments at all
    h0, m0 = hx.search_segments(kmers[:0], np.array([0], np.uint64))
    assert h0.shape == (0, layout[0]) and m0.shape == (0,)
    hx.close()


def test_every_outcome_occurs(orc):
    """over the layout table: segments with a perfect hit, segments with the flag, segments with neither — and all three within one call
    for the layouts whose Bloom filter the planted k-mers cannot fill"""
    seen = np.zeros(3, int)
    for layout in LAYOUTS:
        _, _, _, hits, missing, _ = case(orc, layout)
        o = [int(x.sum()) for x in outcomes(hits, missing)]
        print(layout, "perfect / missing / neither:", o)
        seen += o
        assert o[0] >= 1
        if layout in ((4, 4, 27, 750_000), (256, 4, 31, 1 << 20), (40, 3, 45, 30_011)):
            assert all(o)
    assert all(seen)


@pytest.mark.parametrize("switch", ["upload_chunk_bytes", "dense_report_bytes"])
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[2], LAYOUTS[5]], ids=lambda l: "C%d" % l[0])
def test_chunked_uploads_and_sliced_reports_change_nothing(orc, layout, switch):
    """64 k-mers per upload chunk, or eight segments per slice of the device's counters: segments straddle both kinds of cut"""
    import colorid_amd
    oix, kmers, seg_off, want_hits, want_missing, _ = case(orc, layout)
    n_colors, _, k, _ = layout
    ctx = colorid_amd.Context(0)
    try:
        ctx.tune(switch, 64 * (k + 8) if switch == "upload_chunk_bytes" else 8 * n_colors * 4)
        hx = to_hip_index(ctx, oix)
        got_hits, got_missing = hx.search_segments(kmers, seg_off)
        assert np.array_equal(got_hits, want_hits) and np.array_equal(got_missing, want_missing)
        both = colorid_amd.Context(0)
        try:   # and both at once, through an index that lives in the other context
            both.tune("upload_chunk_bytes", 64 * (k + 8))
            both.tune("dense_report_bytes", 8 * n_colors * 4)
            h = np.zeros_like(want_hits)
            f = np.zeros(len(SEG_LENS), np.uint8)
            rc = both.lib.cid_search_segments(both.h, hx.h, kmers.ctypes.data_as(C.c_void_p), seg_off.ctypes.data_as(C.c_void_p), len(SEG_LENS),
                                              h.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p))
            assert rc == 0
            assert np.array_equal(h, want_hits) and np.array_equal(f.astype(bool), want_missing)
        finally:
            both.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3], LAYOUTS[6]], ids=lambda l: "C%d" % l[0])
def test_device_pointer_form(orc, hip_ctx, layout):
    import torch
    oix, kmers, seg_off, want_hits, want_missing, _ = case(orc, layout)
    n_colors, n_segs = layout[0], len(SEG_LENS)
    hx = to_hip_index(hip_ctx, oix)
    dk = torch.from_numpy(kmers.reshape(-1).copy()).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    d_hits = torch.full((n_segs, n_colors), -559038737, dtype=torch.int32, device="cuda")   # garbage: the call zeroes its outputs
    d_miss = torch.full((n_segs,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, len(kmers), d_hits.data_ptr(), d_miss.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want_hits)
    assert np.array_equal(d_miss.cpu().numpy().astype(bool), want_missing)
    d_hits.fill_(7)
    torch.cuda.synchronize()
    hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, len(kmers), d_hits.data_ptr(), None)   # no flags wanted
    hip_ctx.synchronize()
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want_hits)
    hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), 0, 0, d_hits.data_ptr(), None)                 # nothing to do
    hip_ctx.synchronize()
    hx.close()


def test_errors(orc, hip_ctx):
    import colorid_amd
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    layout = LAYOUTS[1]
    oix, kmers, seg_off, want_hits, want_missing, _ = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    lib, vp = hip_ctx.lib, C.c_void_p

    def code(f):
        with pytest.raises(colorid_amd.CidError) as e:
            f()
        return e.value.code

    def good():
        h, f = hx.search_segments(kmers, seg_off)
        assert np.array_equal(h, want_hits) and np.array_equal(f, want_missing)

    def raw(kmers_p, off_p, n_segs, hits_p):
        return lib.cid_search_segments(hip_ctx.h, hx.h, kmers_p, off_p, n_segs, hits_p, None)

    hits = np.zeros((3, layout[0]), np.uint32)
    off = np.array([0, 1, 2, 3], np.uint64)
    assert raw(kmers.ctypes.data_as(vp), off.ctypes.data_as(vp), 3, None) == INVALID          # null hits
    assert raw(kmers.ctypes.data_as(vp), None, 3, hits.ctypes.data_as(vp)) == INVALID         # null seg_off
    assert raw(None, off.ctypes.data_as(vp), 3, hits.ctypes.data_as(vp)) == INVALID           # null k-mers
    assert lib.cid_search_segments(None, hx.h, kmers.ctypes.data_as(vp), off.ctypes.data_as(vp), 3, hits.ctypes.data_as(vp), None) == INVALID
    good()
    assert code(lambda: hx.search_segments(kmers, np.array([1, 2, 3], np.uint64))) == INVALID         # seg_off[0] != 0
    good()
    assert code(lambda: hx.search_segments(kmers, np.array([0, 5, 3, 9], np.uint64))) == INVALID      # decreasing
    good()
    assert code(lambda: hx.search_segments(kmers, np.array([0, 2, (1 << 32) + 2], np.uint64))) == INVALID   # a segment of 2^32 k-mers
    good()
    fresh = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8)
    assert code(lambda: fresh.search_segments(kmers[:3], off)) == STATE                                # not finalized
    fresh.close()
    mini = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8).set_minimizer(11).finalize()
    assert code(lambda: mini.search_segments(kmers[:3], off)) == UNSUPPORTED                           # a minimizer index
    mini.close()
    wide = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 8193).finalize()
    assert code(lambda: wide.search_segments(kmers[:3], off)) == UNSUPPORTED                           # wide rows
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert code(lambda: wide.search_segments_dev(d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr())) == UNSUPPORTED
    assert code(lambda: hx.search_segments_dev(d.data_ptr(), None, 1, 1, d.data_ptr())) == INVALID
    wide.close()
    good()
    hx.close()


# ------------------------------------------------------------------------------------------------ a wave with several tiles
# Every call above is a few thousand k-mers: four tiles per workgroup, one per wave, so a wave's counters are flushed only at its end.
# The library gives a workgroup n_tiles // (32 * n_cu) tiles once that exceeds four; from 8 on a wave owns two consecutive tiles and
# carries one segment's counters from the first to the second, or flushes between them.  16 384 * n_cu k-mers is the smallest such call.

WALK_PATTERN = [128, 64, 64, 100, 28, 64, 1, 63, 640, 0, 0, 64]     # 19 tiles: the wave pairs fall on it in both phases
WALK_LAYOUTS = [(4, 4, 16, 750_000), (129, 4, 16, 40_009)]          # rs = 1 (narrow); rs = 4 with dead lanes.  k = 16: 16 bytes a k-mer
WALK_POOL = 4096
_walk_cases = {}


def walk_case(orc, layout, n_cu):
    """16 384 * n_cu + 37 k-mers drawn from a pool of 4 096 distinct ones, and what the oracle's answer for every pool k-mer alone (its AND
    word, its absent-row flag) implies per segment.  -> dict, made once: pool, idx (the pool index of every k-mer), seg_off, hits
    [n_segs, C] uint32, missing [n_segs] bool, words [n_segs, w32] uint32 (zero where flagged or empty), and the oracle index.
    Segment s draws from a part of the pool chosen by s % 7: the first quarter is planted into colours c0 and c1, the second into c1 and
    c2, the rest into none — so neighbouring segments have perfect hits in different colours, or none, and only unplanted k-mers can meet
    an absent row."""
    key = (layout, n_cu)
    if key in _walk_cases:
        return _walk_cases[key]
    n_colors, n_hash, k, m = layout
    rng = np.random.default_rng(n_colors * 977 + n_cu)
    n_kmers = 16_384 * n_cu + 37
    reps = n_kmers // sum(WALK_PATTERN) + 1
    lens = np.tile(WALK_PATTERN, reps)
    lens = np.insert(lens, len(WALK_PATTERN) * (reps // 2), 5000)
    n_whole = int(np.searchsorted(np.cumsum(lens), n_kmers, side="right"))      # segments that fit; the next one is cut to the ragged tail
    lens = np.concatenate([lens[:n_whole], [n_kmers - int(lens[:n_whole].sum())], [0]])
    n_segs = len(lens)
    seg_off = np.zeros(n_segs + 1, np.uint64)
    seg_off[1:] = np.cumsum(lens)
    assert int(seg_off[-1]) == n_kmers

    pool = np.unique(random_kmers(rng, WALK_POOL + 64, k), axis=0)[:WALK_POOL]
    assert len(pool) == WALK_POOL
    pool = pool[rng.permutation(WALK_POOL)]
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.3, zero_row_frac=0.002)
    q = WALK_POOL // 4
    c0, c1, c2 = 0, n_colors // 2, n_colors - 1
    for p in range(2 * q):
        for c in ((c0, c1) if p < q else (c1, c2)):
            oix.insert(c, pool[p].tobytes())
    pool_words = np.zeros((WALK_POOL, oix.w32), np.uint32)
    pool_missing = np.zeros(WALK_POOL, bool)
    for p in range(WALK_POOL):
        pool_words[p], pool_missing[p] = oix.search_perfect(pool[p:p + 1])
    pool_bits = np.unpackbits(pool_words.view(np.uint8), axis=1, bitorder="little")[:, :n_colors]
    assert pool_missing.any() and not pool_missing[:2 * q].any()

    lo = np.array([0, 0, q, 0, 0, 0, 0])[np.arange(n_segs) % 7]
    hi = np.array([q, 2 * q, 2 * q, 4 * q, 4 * q, 4 * q, 4 * q])[np.arange(n_segs) % 7]
    idx = (np.repeat(lo, lens) + rng.random(n_kmers) * np.repeat(hi - lo, lens)).astype(np.int64)

    full = np.flatnonzero(lens > 0)                           # reduceat wants strictly increasing starts: the non-empty segments
    starts = seg_off[:-1][full].astype(np.int64)
    missing = np.zeros(n_segs, bool)
    missing[full] = np.logical_or.reduceat(pool_missing[idx], starts)
    words = np.zeros((n_segs, oix.w32), np.uint32)
    words[full] = np.bitwise_and.reduceat(pool_words[idx], starts, axis=0)
    words[missing] = 0
    hits = np.zeros((n_segs, n_colors), np.uint32)
    for b in range(0, len(full), 4096):                       # block-wise over segments: no n_kmers x C array
        blk = full[b:b + 4096]
        k0, k1 = int(seg_off[blk[0]]), int(seg_off[blk[-1] + 1])
        hits[blk] = np.add.reduceat(pool_bits[idx[k0:k1]], starts[b:b + 4096] - k0, axis=0, dtype=np.uint32)
    for a in (pool, idx, seg_off, hits, missing, words):
        a.setflags(write=False)
    _walk_cases[key] = dict(oix=oix, pool=pool, idx=idx, seg_off=seg_off, hits=hits, missing=missing, words=words, colours=(c0, c1, c2))
    return _walk_cases[key]


def check_walk_covers_the_tile_pairs(seg_off, n_cu):
    """the launch gives a wave two tiles, and every way two consecutive tiles of a wave can relate to the segments occurs in it"""
    n_segs, n_kmers = len(seg_off) - 1, int(seg_off[-1])
    n_tiles = (n_kmers + 63) // 64
    tpb = n_tiles // (32 * n_cu)
    assert tpb >= 8                                           # pick_tiles_per_block: 8 tiles a workgroup, two a wave
    per_wave = (tpb + 3) // 4
    first = np.arange(n_tiles, dtype=np.uint64) * 64
    last = np.minimum(first + 63, n_kmers - 1)
    sa = np.searchsorted(seg_off[:n_segs], first, side="right") - 1
    sb = np.searchsorted(seg_off[:n_segs], last, side="right") - 1
    one = sa == sb
    t = np.arange(n_tiles - 1)
    t = t[(t % tpb) % per_wave != per_wave - 1]               # tile t and t + 1 belong to one wave
    a, b = t, t + 1
    seen = {
        "carried without a flush": (one[a] & one[b] & (sa[a] == sa[b])).sum(),
        "flushed between two segments": (one[a] & one[b] & (sa[a] != sa[b]) & (seg_off[sa[a] + 1] == first[b])).sum(),
        "a whole tile, then a boundary tile": (one[a] & ~one[b]).sum(),
        "a boundary tile, then a whole tile": (~one[a] & one[b]).sum(),
        "empty segments at a tile edge": ((np.diff(seg_off) == 0)[:-1] & (seg_off[:-2] % 64 == 0) & (seg_off[:-2] > 0) & (seg_off[:-2] < n_kmers)).sum(),
    }
    print(f"{n_kmers} k-mers, {n_tiles} tiles, {tpb} a workgroup:", seen)
    assert all(seen.values()), seen


@pytest.mark.parametrize("layout", WALK_LAYOUTS, ids=lambda l: "C%d" % l[0])
def test_a_wave_with_several_tiles(orc, hip_ctx, layout):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cs = walk_case(orc, layout, n_cu)
    seg_off, n_segs, n_kmers = cs["seg_off"], len(cs["seg_off"]) - 1, len(cs["idx"])
    check_walk_covers_the_tile_pairs(seg_off, n_cu)
    hx = to_hip_index(hip_ctx, cs["oix"])
    dk = torch.from_numpy(cs["pool"][cs["idx"]].reshape(-1)).cuda()
    do = torch.from_numpy(seg_off.astype(np.int64)).cuda()
    d_hits = torch.full((n_segs, layout[0]), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_miss = torch.full((n_segs,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hx.search_segments_dev(dk.data_ptr(), do.data_ptr(), n_segs, n_kmers, d_hits.data_ptr(), d_miss.data_ptr())
    hip_ctx.synchronize()
    got_hits, got_missing = d_hits.cpu().numpy().view(np.uint32), d_miss.cpu().numpy().astype(bool)
    bad = np.flatnonzero((got_hits != cs["hits"]).any(axis=1))
    print(f"{layout}: {n_segs} segments, {len(bad)} differ in hits, {int((got_missing != cs['missing']).sum())} in the flag; "
          f"{int(cs['missing'].sum())} flagged")
    assert len(bad) == 0, f"segments {bad[:10]} (lengths {np.diff(seg_off)[bad[:10]]})"
    assert np.array_equal(got_missing, cs["missing"])
    lens = np.diff(seg_off).astype(np.int64)
    perfect = (lens > 0) & ~got_missing & (got_hits == lens[:, None]).any(axis=1)
    assert perfect.any() and cs["missing"].any() and ((lens > 0) & ~cs["missing"] & ~perfect).any()
    hx.close()
