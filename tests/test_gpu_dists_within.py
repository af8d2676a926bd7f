"""cid_dists_within through hip.Dists against numpy over the tables of test_gpu_dists.py: every pair (a in the rows asked for, b != a) with
compared >= M and differ <= T — with upper only b > a — as (a, b, differ, compared), sorted by (a, b).  The shapes are those where the 64 x
64 tile, the 32-locus chunk and the 64-bit mask word end; T in {0, 2, L}, M in {1, max(1, L // 2)}, upper on and off.  Row ranges (an
unaligned row0 with upper is the edge of the tile skip), the overflow paths forced by dense_report_bytes (halving down to one row tile,
then the grown list), a cap one short, the count, and the refusals.  Everything is an integer: every comparison is exact, order included."""
import ctypes as C

import numpy as np
import pytest

import within_ref
from test_gpu_dists import table

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 7), (63, 31), (64, 32), (65, 33), (130, 100), (257, 1), (200, 1025)]
INPUTS = [("few", 0.0), ("few", 0.3), ("wide", 0.3)]


def ref(differ, compared, T, M, row0=0, n=None, upper=False):
    """[k, 4] uint32 in (a, b) order: np.nonzero walks the rows, then the columns"""
    A = len(differ)
    n = A - row0 if n is None else n
    d, c = differ[row0:row0 + n].astype(np.int64), compared[row0:row0 + n].astype(np.int64)
    rows, cols = np.arange(row0, row0 + n)[:, None], np.arange(A)[None, :]
    ok = (c >= M) & (d <= T) & ((cols > rows) if upper else (cols != rows))
    a, b = np.nonzero(ok)
    return np.stack([a + row0, b, d[a, b], c[a, b]], 1).astype(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_the_list_equals_numpy(hip_ctx, A, L, alleles, miss):
    import colorid_amd
    codes, differ, compared = table(A, L, alleles, miss)
    d = colorid_amd.Dists(hip_ctx, codes)
    for T in sorted({0, 2, L}):
        for M in sorted({1, max(1, L // 2)}):
            for upper in (True, False):
                want = ref(differ, compared, T, M, upper=upper)
                got = d.within(T, M, upper=upper)
                assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), (T, M, upper)
                assert d.within(T, M, upper=upper).tobytes() == got.tobytes(), (T, M, upper)        # a second call: the same bytes
                assert d.within_count(T, M, upper=upper) == len(want)
                if A >= 3:
                    assert not (got[:, :2] == A - 1).any()                                          # the accession without a call: never
                if alleles == "wide" and A >= 2 and T == 0 and M == 1 and compared[0, 1] >= 1:
                    assert [0, 1] in got[:, :2].tolist()                                            # the identical accessions
    d.close()
    if (A, L) == (65, 33):                                                                          # numpy against the plain loops
        for upper in (True, False):
            assert ref(differ, compared, 2, 1, upper=upper).tolist() == [list(p) for p in within_ref.pairs(differ, compared, 2, 1, upper=upper)]


@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_row_ranges(hip_ctx, A, L):
    import colorid_amd
    codes, differ, compared = table(A, L, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    for row0, n in ((0, A), (1, 1), (63, 2), (64, 66), (A - 1, 1)):
        if row0 < 0 or row0 + n > A:
            continue
        for upper in (True, False):
            for T in (2, L):
                want = ref(differ, compared, T, 1, row0, n, upper)
                assert np.array_equal(d.within(T, 1, row0, n, upper=upper), want), (row0, n, upper, T)
                assert d.within_count(T, 1, row0, n, upper=upper) == len(want)
    for row0 in (0, A):                                                                             # n_rows = 0: a no-op
        assert d.within(L, 1, row0, 0).shape == (0, 4) and d.within_count(L, 1, row0, 0) == 0
    d.close()


def test_overflow_paths(hip_ctx, tune):
    """(130, 100), "few", 0.0, T = L, M = 1, full mode: no cell is missing but the table's all-missing accession and locus, so every ordered
    pair of the other 129 accessions is a hit: 129 x 128 of them, 64 x 128 = 8192 in each full tile of rows"""
    import colorid_amd
    codes, differ, compared = table(130, 100, "few", 0.0)
    want = ref(differ, compared, 100, 1)
    assert len(want) == 129 * 128 and (np.bincount(want[:, 0] // 64) == [64 * 128, 64 * 128, 128]).all()
    d = colorid_amd.Dists(hip_ctx, codes)
    whole = d.within(100, 1)
    tune("dense_report_bytes", 4096)        # a list of 256 entries: three row tiles halve down to one, and one tile's 8192 hits grow the list
    small = d.within(100, 1)
    part = d.within(100, 1, 60, 10, upper=True)
    tune("dense_report_bytes", 1)           # less than one entry: a list of one
    one = d.within(100, 1)
    assert np.array_equal(whole, want) and np.array_equal(small, want) and np.array_equal(one, want)
    assert np.array_equal(part, ref(differ, compared, 100, 1, 60, 10, True))
    # cap one short of the count: n_found is exact, and the second call with room gives the list
    n = C.c_uint64(0)
    out = np.zeros((len(want), 4), np.uint32)
    from colorid_amd._lib import check
    check(d.lib.cid_dists_within(d.h, 0, 130, 100, 1, 0, out.ctypes.data, len(want) - 1, C.byref(n)))
    assert n.value == len(want)
    check(d.lib.cid_dists_within(d.h, 0, 130, 100, 1, 0, out.ctypes.data, n.value, C.byref(n)))
    assert n.value == len(want) and np.array_equal(out, want)
    # cap = 0 with out = NULL: the count alone
    n = C.c_uint64(7)
    check(d.lib.cid_dists_within(d.h, 0, 130, 100, 1, 0, None, 0, C.byref(n)))
    assert n.value == len(want) and d.within_count(100, 1, upper=True) == len(want) // 2
    d.close()


def test_refusals(hip_ctx):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID, check
    d = colorid_amd.Dists(hip_ctx, table(65, 33, "few", 0.3)[0])
    out = np.zeros((8, 4), np.uint32)
    n = C.c_uint64(0)
    bad = [dict(min_compared=0), dict(row0=0, n_rows=66), dict(row0=65, n_rows=1), dict(row0=0xFFFFFFFF, n_rows=2), dict(flags=2), dict(flags=0x80000001),
           dict(out=None)]
    for kw in bad:
        a = dict(row0=0, n_rows=65, max_differ=3, min_compared=1, flags=0, out=out.ctypes.data)
        a.update(kw)
        with pytest.raises(colorid_amd.CidError) as ei:
            check(d.lib.cid_dists_within(d.h, a["row0"], a["n_rows"], a["max_differ"], a["min_compared"], a["flags"], a["out"], 8, C.byref(n)))
        assert ei.value.code == CID_ERR_INVALID, kw
    with pytest.raises(colorid_amd.CidError) as ei:
        check(d.lib.cid_dists_within(d.h, 0, 65, 3, 1, 0, out.ctypes.data, 8, None))                # null n_found
    assert ei.value.code == CID_ERR_INVALID
    assert d.within_count(3, 1) == len(ref(*table(65, 33, "few", 0.3)[1:], 3, 1))                   # the handle is as good as before
    d.close()
