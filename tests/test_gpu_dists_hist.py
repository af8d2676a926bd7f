"""cid_dists_hist through hip.Dists against numpy (tests/hist_ref.py) over the tables of test_gpu_dists.py: over the pairs (a in the rows
asked for, b != a) — with upper only b > a — compared_hist counts them by compared, differ_hist those with compared >= M by differ.  The
shapes are those where the 64 x 64 tile, the 32-locus chunk and the 64-bit mask word end; M in {1, max(1, L // 2)}, upper on and off.
Row ranges (an unaligned row0 with upper is the edge of the tile list), bins past the 4 096 that a workgroup keeps in LDS, several tiles
a workgroup and the flush, and the refusals.  Everything is an integer: every comparison is exact, a second call gives the same bytes."""
import ctypes as C

import numpy as np
import pytest

import hist_ref
from test_gpu_dists import table

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 7), (63, 31), (64, 32), (65, 33), (130, 100), (257, 1), (200, 1025)]
INPUTS = [("few", 0.0), ("few", 0.3), ("wide", 0.3)]


def check_case(d, differ, compared, L, M, upper, row0=0, n=None):
    A = len(differ)
    rows = A - row0 if n is None else n
    want_d, want_c = hist_ref.hist_numpy(differ, compared, L, M, row0, n, upper)
    got_d, got_c = d.hist(M, row0, n, upper=upper)
    what = (M, upper, row0, n)
    assert got_d.dtype == got_c.dtype == np.uint64 and got_d.shape == got_c.shape == (L + 1,), what
    assert np.array_equal(got_c, want_c), what
    assert np.array_equal(got_d, want_d), what
    again_d, again_c = d.hist(M, row0, n, upper=upper)                                          # a second call: the same bytes
    assert again_d.tobytes() == got_d.tobytes() and again_c.tobytes() == got_c.tobytes(), what
    pairs = sum(A - 1 - a for a in range(row0, row0 + rows)) if upper else rows * (A - 1)
    assert int(got_c.sum()) == pairs, what
    assert int(got_d.sum()) == int(got_c[M:].sum()), what
    return got_d, got_c


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_both_histograms_equal_numpy(hip_ctx, A, L, alleles, miss):
    import colorid_amd
    codes, differ, compared = table(A, L, alleles, miss)
    d = colorid_amd.Dists(hip_ctx, codes)
    for M in sorted({1, max(1, L // 2)}):
        for upper in (True, False):
            got_d, _ = check_case(d, differ, compared, L, M, upper)
            running = np.cumsum(got_d)
            for T in sorted({0, 2, L}):
                assert int(running[min(T, L)]) == d.within_count(T, M, upper=upper), (M, upper, T)
    d.close()
    if (A, L) == (65, 33):                                                                      # numpy against the plain loops
        for upper in (True, False):
            dl, cl = hist_ref.hist_loops(differ, compared, L, 2, upper=upper)
            dn, cn = hist_ref.hist_numpy(differ, compared, L, 2, upper=upper)
            assert dn.tolist() == dl and cn.tolist() == cl


@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_row_ranges(hip_ctx, A, L):
    import colorid_amd
    codes, differ, compared = table(A, L, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    for row0, n in ((0, A), (1, 1), (63, 2), (64, 66), (A - 1, 1)):
        if row0 < 0 or row0 + n > A:
            continue
        for upper in (True, False):
            check_case(d, differ, compared, L, 1, upper, row0, n)
    for row0 in (0, A):                                                                         # n_rows = 0: two histograms of zeros
        for upper in (True, False):
            got_d, got_c = d.hist(1, row0, 0, upper=upper)
            assert got_d.shape == got_c.shape == (L + 1,) and not got_d.any() and not got_c.any()
    d.close()


@pytest.mark.parametrize("A,L,miss", [(3, 40_000, 0.0), (3, 40_000, 0.3), (130, 9_000, 0.3)], ids=lambda v: str(v))
def test_bins_past_the_window_in_lds(hip_ctx, A, L, miss):
    """more bins than the 4 096 a workgroup keeps: the counts above go to the global words one by one.  "wide" alleles: nearly every
    shared locus differs, so differ reaches the high bins as compared does (at A = 3 the one comparable pair is the identical one)"""
    import colorid_amd
    codes, differ, compared = table(A, L, "wide", miss)
    off = ~np.eye(A, dtype=bool)
    assert compared[off].max() >= 4096 and (A == 3 or differ[off].max() >= 4096)
    d = colorid_amd.Dists(hip_ctx, codes)
    for M in (1, L // 2):
        for upper in (True, False):
            got_d, got_c = check_case(d, differ, compared, L, M, upper)
            assert got_c[4096:].any() and (A == 3 or got_d[4096:].any() or M > 1)
    d.close()


def test_several_tiles_a_workgroup(hip_ctx):
    """The launch rule: a one-dimensional grid of min(tiles, 3 x the device's compute units) workgroups — 768 on the 256 compute units of an
    MI355X — each with a contiguous share of the tile list.  4 160 accessions are 65 x 65 = 4 225 tiles in full mode, 5 or 6 a workgroup,
    and 65 x 66 / 2 = 2 145 in upper mode, 2 or 3 a workgroup: shares that begin and end inside a row of tiles, bins kept over tiles, one
    flush a workgroup.  Any device of fewer than 715 compute units gives several tiles a workgroup here."""
    import colorid_amd
    A, L = 4160, 8
    codes, differ, compared = table(A, L, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    for upper in (True, False):
        check_case(d, differ, compared, L, 1, upper)
        check_case(d, differ, compared, L, 4, upper)
    check_case(d, differ, compared, L, 1, True, 1000, 3000)                                     # the list begins off a tile's edge
    check_case(d, differ, compared, L, 1, False, 63, 4097)
    d.close()


def test_refusals(hip_ctx):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID, check
    codes, differ, compared = table(65, 33, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    dh, ch = np.zeros(34, np.uint64), np.zeros(34, np.uint64)
    bad = [dict(min_compared=0), dict(row0=0, n_rows=66), dict(row0=65, n_rows=1), dict(row0=0xFFFFFFFF, n_rows=2), dict(flags=2), dict(flags=0x80000001),
           dict(differ=None)]
    for kw in bad:
        a = dict(row0=0, n_rows=65, min_compared=1, flags=0, differ=dh.ctypes.data)
        a.update(kw)
        with pytest.raises(colorid_amd.CidError) as ei:
            check(d.lib.cid_dists_hist(d.h, a["row0"], a["n_rows"], a["min_compared"], a["flags"], a["differ"], ch.ctypes.data))
        assert ei.value.code == CID_ERR_INVALID, kw
    with pytest.raises(colorid_amd.CidError) as ei:
        check(d.lib.cid_dists_hist(None, 0, 65, 1, 0, dh.ctypes.data, ch.ctypes.data))          # null handle
    assert ei.value.code == CID_ERR_INVALID
    dh[:] = 7
    check(d.lib.cid_dists_hist(d.h, 0, 65, 1, 1, dh.ctypes.data, None))                         # compared_hist = NULL: differ_hist alone
    want_d, want_c = hist_ref.hist_numpy(differ, compared, 33, 1, upper=True)
    assert np.array_equal(dh, want_d)
    got_d, got_c = d.hist(1, upper=True)                                                        # the handle is as good as before
    assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c)
    d.close()
