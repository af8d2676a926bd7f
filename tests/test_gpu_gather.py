"""cid_search_gather / cid_search_gather_set against tests/gather_ref.py on the oracle's bits: P[k] is the oracle's perfect search of query
k-mer k alone (its AND word, unpacked), freq is random in 1..50, and every field of every row, n_out and n_hit must be equal.

The index is random_index at a density whose chance hits are background (0.02: about 2 of 5 000 k-mers per colour with two hashes, none
with three or four).  Into it go overlapping stretches of the 5 000 query k-mers, in colours whose background is cleared first so that
what the test plants is what the colours hold (Bloom collisions of the planted k-mers aside):
    A       u k-mers [0, 15u/10)            the first pick
    TWIN    the same k-mers in a higher colour: an identical column, a tie at every round until A goes, never emitted
    SUB     [u/10, 4u/10), inside A: empty once A is gone, never emitted
    B       [u, 22u/10) in the HIGHEST colour: overlaps A, so its new_kmers is below its total_kmers
    D, E    [2u, 26u/10) and [25u/10, 28u/10), in colours 63 and 64 where the index has them
with u = min(1000, bloom_size / 10); the four-colour layout holds A, TWIN, D and B.  The query is then shuffled, so that every prefix of
it (the k-mer counts around the 64-row tile) holds k-mers of every stretch."""
import ctypes as C

import numpy as np
import pytest

import gather_ref
from util import random_index, random_kmers, to_hip_index

gpu = pytest.mark.gpu

# (n_colors, n_hash, k, bloom_size): test_gpu_cover.py's
LAYOUTS = [
    (4, 4, 27, 750_000),        # rs = 1
    (129, 4, 31, 40_009),       # dead lanes, rs = 4
    (1024, 2, 31, 10_007),
    (8192, 2, 31, 1_009),
    (40, 3, 45, 30_011),        # k > 32
]
N_QUERY = 5000
COUNTS = [0, 1, 63, 64, 65, N_QUERY]       # around the 64-row tile; 5 000 rows span several workgroups
INVALID, UNSUPPORTED, STATE = -1, -4, -5
ids = lambda l: "C%d-n%d-k%d-m%d" % l
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

_cases = {}


def max_rows_of(layout):
    return None if layout[0] <= 129 else 40          # wide layouts: the cap is exercised and the numpy reference stays at seconds


def planted_colours(n_colors):
    """{name: colour}"""
    if n_colors <= 4:
        return dict(A=0, TWIN=1, D=2, B=n_colors - 1)            # no room for SUB and E: three rows, the third one D's
    pc = dict(A=1, TWIN=5, SUB=7, B=n_colors - 1)
    if n_colors > 64:
        pc.update(D=63, E=64)
    else:
        pc.update(D=20, E=21)
    return pc


def case(orc, layout):
    """(oracle index, canonical query k-mers, freq, P): made once per layout and left unchanged"""
    if layout in _cases:
        return _cases[layout]
    n_colors, n_hash, k, m = layout
    rng = np.random.default_rng(n_colors * 31 + k)
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.02, zero_row_frac=0.2)
    raw = random_kmers(rng, N_QUERY, k)
    canon = sorted({min(b, b.translate(_COMP)[::-1]) for b in (r.tobytes() for r in raw)})      # distinct and canonical: a set holds them as they are
    assert len(canon) == N_QUERY
    kmers = np.frombuffer(b"".join(canon), np.uint8).reshape(N_QUERY, k).copy()
    kmers = kmers[rng.permutation(N_QUERY)]
    order = rng.permutation(N_QUERY)                 # stretch position -> query row
    pc = planted_colours(n_colors)
    rows = oix.rows()
    for c in pc.values():                            # no background in the planted colours
        rows[:, c // 32] &= ~np.uint32(1 << (c % 32))
    u = min(1000, m // 10)
    stretch = dict(A=(0, 15 * u // 10), TWIN=(0, 15 * u // 10), SUB=(u // 10, 4 * u // 10), B=(u, 22 * u // 10), D=(2 * u, 26 * u // 10),
                   E=(25 * u // 10, 28 * u // 10))
    for name, c in pc.items():
        a, b = stretch[name]
        for i in order[a:b]:
            oix.insert(c, kmers[i].tobytes())
    freq = rng.integers(1, 51, N_QUERY).astype(np.uint32)
    P = np.zeros((N_QUERY, n_colors), bool)
    for i in range(N_QUERY):
        words = oix.search_perfect(kmers[i:i + 1])[0]
        P[i] = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_colors]
    for a in (kmers, freq, P):
        a.setflags(write=False)
    _cases[layout] = (oix, kmers, freq, P)
    return _cases[layout]


_refs = {}


def ref(orc, layout, n, min_new=1):
    key = (layout, n, min_new)
    if key not in _refs:
        _, _, freq, P = case(orc, layout)
        _refs[key] = gather_ref.gather(P[:n], freq[:n], min_new, max_rows_of(layout))
    return _refs[key]


def assert_rows_equal(got, want, what=""):
    """got: (array of GATHER_DTYPE, n_hit); want: gather_ref's (rows, n_hit, ties)"""
    rows, n_hit = got
    wrows, wn_hit, _ = want
    assert n_hit == wn_hit, f"{what}n_hit {n_hit}, want {wn_hit}"
    assert len(rows) == len(wrows), f"{what}n_out {len(rows)}, want {len(wrows)}"
    for f in gather_ref.FIELDS:
        g, w = [int(x) for x in rows[f]], [r[f] for r in wrows]
        bad = [i for i in range(len(w)) if g[i] != w[i]]
        assert not bad, f"{what}{f}: rows {bad[:5]} differ: got {[g[i] for i in bad[:5]]}, want {[w[i] for i in bad[:5]]}"
    assert not rows["reserved"].any()


def make_set(hip_ctx, kmers, freq, k):
    """a finalized set that holds k-mer i freq[i] times"""
    import colorid_amd
    ks = colorid_amd.KmerSet(hip_ctx, k)
    seqs = []
    for i in range(len(kmers)):
        seqs += [kmers[i].tobytes()] * int(freq[i])
    if seqs:
        ks.add_seqs(seqs)
    ks.finalize()
    return ks


def test_the_planting_shows_every_outcome(orc):
    """on the REFERENCE values, so that an unlucky index cannot make the comparison vacuous: at least 4 rows, a row that adds less than
    its accession holds, a colour with hits that is never emitted, a tie at selection time, weights that differ from counts"""
    for layout in LAYOUTS:
        n_colors = layout[0]
        _, _, freq, P = case(orc, layout)
        rows, n_hit, ties = ref(orc, layout, N_QUERY)
        emitted = {r["colour"] for r in rows}
        never = [c for c in range(n_colors) if P[:, c].any() and c not in emitted]
        pc = planted_colours(n_colors)
        print(layout, "rows", len(rows), "n_hit", n_hit, "first rows", [(r["colour"], r["new_kmers"], r["total_kmers"]) for r in rows[:6]],
              "ties", ties[:6], "never emitted", len(never))
        assert rows[0]["colour"] == pc["A"] and ties[0] >= 2                       # A and its twin
        assert pc["TWIN"] in never and pc["B"] in emitted
        assert any(r["new_kmers"] < r["total_kmers"] for r in rows)
        assert any(r["new_weight"] != r["new_kmers"] for r in rows)
        if max_rows_of(layout) is None and "SUB" in pc:
            assert pc["SUB"] in never                                             # run to exhaustion, and still absent
        assert pc["D"] in emitted
        if n_colors > 4:                                                          # four colours, one of them a twin: three rows at most
            assert len(rows) >= 4 and pc["E"] in emitted
        if max_rows_of(layout) is not None:
            assert len(rows) == 40                                                # the cap ends these


@gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_gather_matches_the_reference(orc, hip_ctx, layout, n):
    oix, kmers, freq, P = case(orc, layout)
    k = layout[2]
    hx = to_hip_index(hip_ctx, oix)
    want = ref(orc, layout, n)
    mr = max_rows_of(layout)
    assert_rows_equal(hx.search_gather(kmers[:n], freq[:n], 1, mr), want, "host form: ")
    ks = make_set(hip_ctx, kmers[:n], freq[:n], k)
    assert ks.as_dict() == {kmers[i].tobytes(): int(freq[i]) for i in range(n)}
    assert_rows_equal(ks.search_gather(hx, 1, mr), want, "set form: ")
    # no multiplicities: every k-mer weighs 1
    assert_rows_equal(hx.search_gather(kmers[:n], None, 1, mr), gather_ref.gather(P[:n], None, 1, mr), "freq = NULL: ")
    # max_rows = 0: nothing emitted, n_hit still counted
    rows, n_hit = hx.search_gather(kmers[:n], freq[:n], 1, 0)
    assert len(rows) == 0 and n_hit == want[1]
    ks.close()
    hx.close()


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_min_new_and_max_rows_end_the_cover(orc, hip_ctx, layout):
    oix, kmers, freq, P = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    full = ref(orc, layout, N_QUERY)[0]
    mr = max_rows_of(layout)
    min_new = full[2]["new_kmers"]
    want = ref(orc, layout, N_QUERY, min_new)
    assert 3 <= len(want[0]) <= len(full)
    assert_rows_equal(hx.search_gather(kmers, freq, min_new, mr), want, "min_new = the third row's: ")
    ks = make_set(hip_ctx, kmers, freq, layout[2])
    assert_rows_equal(ks.search_gather(hx, min_new, mr), want, "set form, min_new = the third row's: ")
    assert_rows_equal(ks.search_gather(hx, 1, 2), gather_ref.gather(P, freq, 1, 2), "max_rows = 2: ")
    assert_rows_equal(hx.search_gather(kmers, freq, N_QUERY + 1, mr), gather_ref.gather(P, freq, N_QUERY + 1, mr), "min_new above every count: ")
    ks.close()
    hx.close()


@gpu
def test_chunked_uploads_change_nothing(orc, layout=LAYOUTS[1]):
    """64 k-mers per upload chunk: the matrix is filled by 79 launches of the rows kernel"""
    import colorid_amd
    oix, kmers, freq, _ = case(orc, layout)
    ctx = colorid_amd.Context(0)
    try:
        hx = to_hip_index(ctx, oix)
        ctx.tune("upload_chunk_bytes", 64 * (layout[2] + 8))
        assert_rows_equal(hx.search_gather(kmers, freq), ref(orc, layout, N_QUERY), "chunked: ")
    finally:
        ctx.close()


@gpu
def test_kmers_with_empty_rows(orc, hip_ctx):
    """an index without a bit: every row of the matrix is empty, nothing is emitted and nothing hits — and the k-mers stay live"""
    import colorid_amd
    layout = LAYOUTS[1]
    _, kmers, freq, _ = case(orc, layout)
    hx = colorid_amd.Index(hip_ctx, 1000, 2, layout[2], 70).finalize()
    for n in (1, 64, 1000):
        rows, n_hit = hx.search_gather(kmers[:n], freq[:n])
        assert len(rows) == 0 and n_hit == 0
    ks = make_set(hip_ctx, kmers[:200], freq[:200], layout[2])
    rows, n_hit = ks.search_gather(hx)
    assert len(rows) == 0 and n_hit == 0
    ks.close()
    hx.close()


@gpu
def test_errors(orc, hip_ctx):
    import colorid_amd
    layout = LAYOUTS[1]
    n_colors, _, k, _ = layout
    oix, kmers, freq, _ = case(orc, layout)
    hx = to_hip_index(hip_ctx, oix)
    ks = make_set(hip_ctx, kmers[:100], freq[:100], k)
    lib, vp = hip_ctx.lib, C.c_void_p
    p = lambda a: a.ctypes.data_as(vp)
    out = np.zeros(n_colors, colorid_amd.hip.GATHER_DTYPE)
    n_out, n_hit = C.c_size_t(0), C.c_uint64(0)
    ro, rh = C.byref(n_out), C.byref(n_hit)

    def code(f):
        with pytest.raises(colorid_amd.CidError) as e:
            f()
        return e.value.code

    g, gs = lib.cid_search_gather, lib.cid_search_gather_set
    assert g(None, hx.h, p(kmers), p(freq), 100, 1, 10, p(out), ro, rh) == INVALID
    assert g(hip_ctx.h, None, p(kmers), p(freq), 100, 1, 10, p(out), ro, rh) == INVALID
    assert g(hip_ctx.h, hx.h, None, p(freq), 100, 1, 10, p(out), ro, rh) == INVALID            # null k-mers
    assert g(hip_ctx.h, hx.h, p(kmers), p(freq), 100, 1, 10, None, ro, rh) == INVALID          # null out
    assert g(hip_ctx.h, hx.h, p(kmers), p(freq), 100, 1, 10, p(out), None, rh) == INVALID
    assert g(hip_ctx.h, hx.h, p(kmers), p(freq), 100, 1, 10, p(out), ro, None) == INVALID
    assert g(hip_ctx.h, hx.h, p(kmers), p(freq), 100, 0, 10, p(out), ro, rh) == INVALID        # min_new = 0
    assert gs(None, hx.h, ks.h, 1, 10, p(out), ro, rh) == INVALID
    assert gs(hip_ctx.h, None, ks.h, 1, 10, p(out), ro, rh) == INVALID
    assert gs(hip_ctx.h, hx.h, None, 1, 10, p(out), ro, rh) == INVALID                         # null set
    assert gs(hip_ctx.h, hx.h, ks.h, 1, 10, None, ro, rh) == INVALID
    assert gs(hip_ctx.h, hx.h, ks.h, 1, 10, p(out), None, rh) == INVALID
    assert gs(hip_ctx.h, hx.h, ks.h, 1, 10, p(out), ro, None) == INVALID
    assert gs(hip_ctx.h, hx.h, ks.h, 0, 10, p(out), ro, rh) == INVALID
    open_set = colorid_amd.KmerSet(hip_ctx, k)
    assert code(lambda: open_set.search_gather(hx)) == STATE                                   # set not finalized
    open_set.close()
    other_k = make_set(hip_ctx, kmers[:10, :21], freq[:10], 21)
    assert code(lambda: other_k.search_gather(hx)) == INVALID                                  # a set of another k
    other_k.close()
    fresh = colorid_amd.Index(hip_ctx, 1000, 2, k, 8)
    assert code(lambda: fresh.search_gather(kmers[:3])) == STATE                               # index not finalized
    assert code(lambda: ks.search_gather(fresh)) == STATE
    fresh.close()
    mini = colorid_amd.Index(hip_ctx, 1000, 2, k, 8).set_minimizer(11).finalize()
    assert code(lambda: mini.search_gather(kmers[:3])) == UNSUPPORTED                          # a minimizer index
    assert code(lambda: ks.search_gather(mini)) == UNSUPPORTED
    mini.close()
    wide = colorid_amd.Index(hip_ctx, 1000, 2, k, 8193).finalize()
    assert code(lambda: wide.search_gather(kmers[:3])) == UNSUPPORTED                          # more than 8192 colours
    assert code(lambda: ks.search_gather(wide)) == UNSUPPORTED
    wide.close()
    assert_rows_equal(hx.search_gather(kmers, freq), ref(orc, layout, N_QUERY), "after the refusals: ")
    ks.close()
    hx.close()
