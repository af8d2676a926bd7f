"""cid_dists_best / cid_dists_forest through hip.Dists against tests/mst_ref.py (Kruskal over the sorted edges) and a numpy argmin, on the
tables of test_gpu_dists.py: shapes around the 64 x 64 tile and the 32-locus chunk, alleles from {1, 2, 3} (ties everywhere: a round
without a strict order builds cycles here) and from a wide range, missing rates 0 and 0.3, identical accessions, an accession and a locus
without a call.  Constructed forests over three tiles (A = 130): a star, a path, two trees, one edge removed by min_compared.  Everything is
integer arithmetic and the edge key is a strict total order: every comparison is exact.

The packing limit (2 ceil(log2(L + 1)) + ceil(log2 A) <= 64) cannot be crossed by a table that fits a device: the smallest shape past it,
2^30 loci x 5 accessions, is 256 GiB of transposed codes (the accession stride is padded to 64) and 20 GiB on the host, so cid_dists_create
refuses it first and the CID_ERR_UNSUPPORTED of cid_dists_best / cid_dists_forest is not reachable from a test.  What is tested is the
large-L side inside the limit: A = 2, L = 2^20 + 1 gives the right edge."""
import functools

import numpy as np
import pytest

import mst_ref
from test_gpu_dists import INPUTS, SHAPES, table

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def reference(A, L, alleles, miss, M):
    _, differ, compared = table(A, L, alleles, miss)
    return mst_ref.forest(differ.astype(np.int64), compared.astype(np.int64), M)


def as_tuples(edges):
    return [tuple(int(v) for v in e) for e in edges]


def max_rounds(A):
    return (A - 1).bit_length() + 1          # ceil(log2 A) + 1


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_forest_equals_kruskal(hip_ctx, A, L, alleles, miss):
    import colorid_amd
    codes, differ, compared = table(A, L, alleles, miss)
    d = colorid_amd.Dists(hip_ctx, codes)
    for M in sorted({1, 2, L}):
        want = reference(A, L, alleles, miss, M)
        edges, rounds = d.forest(M)
        assert as_tuples(edges) == want, M
        assert len(edges) == A - len(set(mst_ref.components(A, want)))
        assert rounds <= max_rounds(A) and (rounds >= 1 or A == 1), (M, rounds)
    # the resident arrays are untouched: the rows are what they were
    got_d, got_c = d.rows()
    d.close()
    assert np.array_equal(got_d, differ) and np.array_equal(got_c, compared)


def numpy_best(differ, compared, comp, M, L):
    """per row the argmin of (differ, L - compared, j) over the j of another label with compared >= M"""
    A = len(differ)
    differ, compared = differ.astype(np.int64), compared.astype(np.int64)
    key = (differ * (L + 1) + (L - compared)) * A + np.arange(A)[None, :]
    ok = (comp[None, :] != comp[:, None]) & (compared >= M)
    key[~ok] = np.iinfo(np.int64).max
    j = key.argmin(1)
    none = ~ok.any(1)
    rows = np.arange(A)
    b = np.where(none, NONE, j).astype(np.uint32)
    return b, np.where(none, 0, differ[rows, j]).astype(np.uint32), np.where(none, 0, compared[rows, j]).astype(np.uint32)


def labellings(A):
    i = np.arange(A, dtype=np.uint32)
    rng = np.random.default_rng(A)
    odd = np.array([0xFFFFFFFF, 0x80000000, 7, 0xFFFFFFFE], np.uint32)
    return {"identity": i, "all_equal": np.full(A, 5, np.uint32), "interleaved": i % 2, "blocks_aligned": i // 64,
            "blocks_misaligned": (i + 23) // 64, "not_small": odd[rng.integers(0, 4, size=A)]}


@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_best_equals_a_numpy_argmin(hip_ctx, A, L):
    import colorid_amd
    for alleles, miss in (("few", 0.0), ("few", 0.3), ("wide", 0.3)):
        codes, differ, compared = table(A, L, alleles, miss)
        d = colorid_amd.Dists(hip_ctx, codes)
        for name, comp in labellings(A).items():
            for M in sorted({1, 2, L}):
                got = d.best(comp, M)
                want = numpy_best(differ, compared, comp, M, L)
                for g, w, what in zip(got, want, ("b", "differ", "compared")):
                    assert np.array_equal(g, w), (alleles, miss, name, M, what)
                if name == "all_equal":
                    assert (got[0] == NONE).all() and not got[1].any() and not got[2].any()
                if name == "identity":     # the `nearest` rule of clusters.tsv
                    near = mst_ref.nearest(differ.astype(np.int64), compared.astype(np.int64), M) if A <= 65 else None
                    if near is not None:
                        assert [None if b == NONE else (int(b), int(x), int(c)) for b, x, c in zip(*got)] == near
        d.close()


def forest_of(hip_ctx, codes, M=1):
    import colorid_amd
    d = colorid_amd.Dists(hip_ctx, np.asarray(codes, np.uint32))
    edges, rounds = d.forest(M)
    d.close()
    return as_tuples(edges), rounds


def test_identical_accessions_give_the_star_on_the_first(hip_ctx):
    edges, rounds = forest_of(hip_ctx, np.full((130, 5), 3))
    assert edges == [(0, j, 0, 5) for j in range(1, 130)] and rounds <= max_rounds(130)


def test_a_chain_gives_the_path(hip_ctx):
    A = 130
    codes = np.ones((A, A - 1), np.uint32)
    for i in range(1, A):
        codes[i:, i - 1] = 2                 # accession i differs from i - 1 at locus i - 1, a new one: differ(i, j) = |i - j|
    edges, rounds = forest_of(hip_ctx, codes)
    assert edges == [(i, i + 1, 1, A - 1) for i in range(A - 1)]
    assert 1 <= rounds <= max_rounds(A)


def test_two_groups_on_disjoint_loci_give_two_trees(hip_ctx):
    A, L = 130, 40
    rng = np.random.default_rng(130)
    codes = rng.integers(1, 4, size=(A, L)).astype(np.uint32)
    group = (np.arange(A) % 3 == 0)          # interleaved over the tiles
    codes[group, L // 2:] = 0
    codes[~group, :L // 2] = 0
    differ, compared = mst_ref.matrices(codes)
    edges, rounds = forest_of(hip_ctx, codes)
    assert edges == mst_ref.forest(differ, compared, 1)
    assert len(edges) == A - 2 and all(group[lo] == group[hi] for lo, hi, _, _ in edges)
    assert sorted(set(mst_ref.components(A, edges))) == [0, 1] and rounds <= max_rounds(A)


def test_min_compared_between_two_pairs_removes_one_edge(hip_ctx):
    A, L = 130, 10
    codes = np.ones((A, L), np.uint32)
    codes[129, 3:] = 0                       # the last accession shares 3 loci with everyone, the others share 10
    with_it, _ = forest_of(hip_ctx, codes, 3)
    without, _ = forest_of(hip_ctx, codes, 4)
    assert with_it == [(0, j, 0, 10) for j in range(1, 129)] + [(0, 129, 0, 3)]
    assert without == with_it[:-1]


def test_a_large_locus_count_inside_the_packing_limit(hip_ctx):
    import colorid_amd
    L = (1 << 20) + 1                        # 21 bits of differ, 21 of L - compared, 1 of j
    codes = np.ones((2, L), np.uint32)
    codes[1, ::3] = 2
    codes[1, 5::1000] = 0
    codes[0, L - 1] = 0
    called = (codes[0] != 0) & (codes[1] != 0)
    want = (0, 1, int((called & (codes[0] != codes[1])).sum()), int(called.sum()))
    d = colorid_amd.Dists(hip_ctx, codes)
    edges, rounds = d.forest()
    b, differ, compared = d.best(np.array([9, 4], np.uint32), want[3])
    nothing = d.best(np.array([9, 4], np.uint32), want[3] + 1)
    d.close()
    assert as_tuples(edges) == [want] and rounds == 1
    assert b.tolist() == [1, 0] and differ.tolist() == [want[2]] * 2 and compared.tolist() == [want[3]] * 2
    assert nothing[0].tolist() == [NONE, NONE]


def test_errors(hip_ctx):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID, check
    import ctypes as C
    d = colorid_amd.Dists(hip_ctx, table(65, 33, "few", 0.3)[0])
    comp = np.arange(65, dtype=np.uint32)
    out = np.zeros((65, 4), np.uint32)
    n, r = C.c_uint32(0), C.c_uint32(0)
    calls = [lambda: d.best(comp, 0), lambda: d.forest(0),
             lambda: check(d.lib.cid_dists_best(None, comp.ctypes.data, 1, out.ctypes.data)),
             lambda: check(d.lib.cid_dists_best(d.h, None, 1, out.ctypes.data)),
             lambda: check(d.lib.cid_dists_best(d.h, comp.ctypes.data, 1, None)),
             lambda: check(d.lib.cid_dists_forest(None, 1, out.ctypes.data, C.byref(n), C.byref(r))),
             lambda: check(d.lib.cid_dists_forest(d.h, 1, None, C.byref(n), C.byref(r))),
             lambda: check(d.lib.cid_dists_forest(d.h, 1, out.ctypes.data, None, C.byref(r))),
             lambda: check(d.lib.cid_dists_forest(d.h, 1, out.ctypes.data, C.byref(n), None))]
    for k, call in enumerate(calls):
        with pytest.raises(colorid_amd.CidError) as ei:
            call()
        assert ei.value.code == CID_ERR_INVALID, k
    edges, _ = d.forest()                    # the object is as good as before
    d.close()
    assert as_tuples(edges) == reference(65, 33, "few", 0.3, 1)
