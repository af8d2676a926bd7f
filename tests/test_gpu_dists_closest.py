"""cid_dists_closest through hip.Dists against tests/closest_ref.py over the tables of test_gpu_dists.py: per accession a of the rows asked
for, its K nearest among the b != a with compared >= M and differ <= T, by (differ, more compared first, b), as (a, b, differ, compared),
and (a, 0xFFFFFFFF, 0, 0) past the last candidate.  The shapes are those where the 64 x 64 tile, the 32-locus chunk and the 64-bit mask
word end; K in {1, 3, 64}, T in {2, unbounded}, M in {1, max(1, L // 2)}.  What these tables hold — ties at the cut that only the column
decides, short rows, rows merged from several column tiles — is asserted in test_closest_ref_cpu.py.  Against cid_dists_best (K = 1) and
cid_dists_within (sorted and cut); row ranges; slices forced by dense_report_bytes; the refusals.  Everything is an integer: every
comparison is exact, order included."""
import functools

import numpy as np
import pytest

import closest_ref
from test_gpu_dists import table

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 7), (63, 31), (64, 32), (65, 33), (130, 100), (257, 1), (200, 1025)]
INPUTS = [("few", 0.0), ("few", 0.3), ("wide", 0.3)]
UNBOUNDED = closest_ref.UNBOUNDED


@functools.lru_cache(maxsize=None)
def ref(A, L, alleles, miss, K, T, M):
    """[A, K, 4] uint32 from the plain loops: computed once per table and parameters, shared and left unchanged"""
    _, differ, compared = table(A, L, alleles, miss)
    out = np.array(closest_ref.closest(differ.tolist(), compared.tolist(), K, None if T == UNBOUNDED else T, M), np.uint32).reshape(A, K, 4)
    out.setflags(write=False)
    return out


def cut_of_within(pairs, row0, n, K):
    """[n, K, 4]: per row its part of a cid_dists_within list, sorted by (differ, -compared, b) and cut at K"""
    out = np.zeros((n, K, 4), np.uint32)
    out[:, :, 0] = np.arange(row0, row0 + n, dtype=np.uint32)[:, None]
    out[:, :, 1] = closest_ref.NONE
    for a in range(row0, row0 + n):
        mine = pairs[pairs[:, 0] == a].astype(np.int64)
        mine = mine[np.lexsort((mine[:, 1], -mine[:, 3], mine[:, 2]))][:K]
        out[a - row0, :len(mine)] = mine
    return out


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_the_k_nearest_equal_the_reference(hip_ctx, A, L, alleles, miss):
    import colorid_amd
    codes, differ, compared = table(A, L, alleles, miss)
    d = colorid_amd.Dists(hip_ctx, codes)
    for T in (2, UNBOUNDED):
        for M in sorted({1, max(1, L // 2)}):
            pairs = d.within(T, M, upper=False)
            for K in (1, 3, 64):
                want = ref(A, L, alleles, miss, K, T, M)
                got = d.closest(K, T, M)
                assert got.dtype == np.uint32 and got.shape == (A, K, 4) and np.array_equal(got, want), (K, T, M)
                assert d.closest(K, T, M).tobytes() == got.tobytes(), (K, T, M)                     # a second call: the same bytes
                assert np.array_equal(got, cut_of_within(pairs, 0, A, K)), (K, T, M)
                if A >= 3:
                    assert (got[A - 1, :, 1] == closest_ref.NONE).all() and not (got[:, :, 1] == A - 1).any()   # the accession without a call
            b, bd, bc = d.best(np.arange(A), M)                                                     # every accession its own component
            one = d.closest(1, UNBOUNDED, M)
            assert np.array_equal(one[:, 0, 1], b) and np.array_equal(one[:, 0, 2], bd) and np.array_equal(one[:, 0, 3], bc), M
    if alleles == "wide" and A >= 2 and compared[0, 1] >= 1:
        first = d.closest(1)[:2, 0]
        assert first[0].tolist() == [0, 1, 0, compared[0, 1]] and first[1].tolist() == [1, 0, 0, compared[0, 1]]   # the identical accessions
    d.close()


@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_row_ranges(hip_ctx, A, L):
    import colorid_amd
    codes, differ, compared = table(A, L, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    for row0, n in ((0, A), (1, 1), (63, 2), (64, 66), (A - 1, 1)):
        if row0 < 0 or row0 + n > A:
            continue
        for K in (1, 3, 64):
            for T in (2, UNBOUNDED):
                want = ref(A, L, "few", 0.3, K, T, 1)[row0:row0 + n]
                assert np.array_equal(d.closest(K, T, 1, row0, n), want), (row0, n, K, T)
    for row0 in (0, A):                                                                             # n_rows = 0: a no-op
        assert d.closest(3, UNBOUNDED, 1, row0, 0).shape == (0, 3, 4)
    from colorid_amd._lib import check
    check(d.lib.cid_dists_closest(d.h, A, 0, 3, UNBOUNDED, 1, None))                                # ... that needs no out
    d.close()


def test_slices_forced_by_dense_report_bytes(hip_ctx, tune):
    """(130, 100): three row tiles x three column tiles.  part is K x 3 x 8 bytes a row: 4096 bytes hold one row tile at K = 1 and less
    than one at K = 3 and 64 (a slice is one tile all the same), 1 byte holds nothing"""
    import colorid_amd
    codes, differ, compared = table(130, 100, "few", 0.0)
    d = colorid_amd.Dists(hip_ctx, codes)
    whole = {(K, T): d.closest(K, T) for K in (1, 3, 64) for T in (2, UNBOUNDED)}
    part_whole = d.closest(3, UNBOUNDED, 1, 60, 70)
    for budget in (4096, 1):
        tune("dense_report_bytes", budget)
        for (K, T), want in whole.items():
            assert np.array_equal(d.closest(K, T), want), (budget, K, T)
        assert np.array_equal(d.closest(3, UNBOUNDED, 1, 60, 70), part_whole), budget
    for (K, T), want in whole.items():
        assert np.array_equal(want, ref(130, 100, "few", 0.0, K, T, 1)), (K, T)
    d.close()


def test_refusals(hip_ctx):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID, CID_ERR_UNSUPPORTED, check
    d = colorid_amd.Dists(hip_ctx, table(65, 33, "few", 0.3)[0])
    out = np.full((65 * 65, 4), 7, np.uint32)
    want = ref(65, 33, "few", 0.3, 3, UNBOUNDED, 1)
    bad = [(dict(k=0), CID_ERR_INVALID), (dict(min_compared=0), CID_ERR_INVALID), (dict(row0=0, n_rows=66), CID_ERR_INVALID),
           (dict(row0=65, n_rows=1), CID_ERR_INVALID), (dict(row0=0xFFFFFFFF, n_rows=2), CID_ERR_INVALID), (dict(out=None), CID_ERR_INVALID),
           (dict(k=65), CID_ERR_UNSUPPORTED), (dict(k=0xFFFFFFFF), CID_ERR_UNSUPPORTED)]
    for kw, code in bad:
        a = dict(row0=0, n_rows=65, k=3, max_differ=UNBOUNDED, min_compared=1, out=out.ctypes.data)
        a.update(kw)
        with pytest.raises(colorid_amd.CidError) as ei:
            check(d.lib.cid_dists_closest(d.h, a["row0"], a["n_rows"], a["k"], a["max_differ"], a["min_compared"], a["out"]))
        assert ei.value.code == code, kw
        if code == CID_ERR_UNSUPPORTED:
            assert "at most 64" in str(ei.value)                                                       # the limit is in the message
        assert (out == 7).all(), kw                                                                 # refused before anything is written
        assert np.array_equal(d.closest(3), want), kw                                               # the handle is as good as before
    with pytest.raises(colorid_amd.CidError) as ei:
        check(d.lib.cid_dists_closest(None, 0, 0, 3, UNBOUNDED, 1, out.ctypes.data))                # null handle
    assert ei.value.code == CID_ERR_INVALID
    d.close()
