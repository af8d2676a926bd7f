"""cid_dists_create / cid_dists_rows through hip.Dists against numpy: compared = called @ called.T, differ = both called and unequal codes.
Shapes around the 64 x 64 tile and the 32-locus chunk (one cell, tile - 1 / tile / tile + 1, several tiles, one locus, a locus count past a
mask word and a chunk), alleles from {1, 2, 3} (equal calls are frequent) and from a wide range with 0xFFFFFFFD, missing rates 0 and 0.3,
and in every table that has room an all-missing accession, two identical accessions and an all-missing locus.  Row blocks, compared =
NULL, slices forced by dense_report_bytes, and the refusals.  The counts are integers: every comparison is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 7), (63, 31), (64, 32), (65, 33), (130, 100), (257, 1), (200, 1025)]
INPUTS = [("few", 0.0), ("few", 0.3), ("wide", 0.0), ("wide", 0.3)]


@functools.lru_cache(maxsize=None)
def table(A, L, alleles, miss):
    """(codes, differ, compared): the reference is computed once per table and shared"""
    rng = np.random.default_rng([A, L, int(alleles == "wide"), int(miss * 10)])
    if alleles == "few":
        codes = rng.integers(1, 4, size=(A, L), dtype=np.uint32)
    else:
        codes = rng.choice(np.array([1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFC, 0xFFFFFFFD], np.uint32), size=(A, L))
        anywhere = rng.integers(1, 0xFFFFFFFE, size=(A, L), dtype=np.uint32)      # 1 .. 0xFFFFFFFD
        pick = rng.random((A, L)) < 0.5
        codes[pick] = anywhere[pick]
    codes[rng.random((A, L)) < miss] = 0
    if alleles == "wide":
        codes[0, 0] = 0xFFFFFFFD     # the largest code there is
    if A >= 2:
        codes[1] = codes[0]          # two identical accessions
    if A >= 3:
        codes[A - 1] = 0             # an accession without a call
    if L >= 2:
        codes[:, L - 1] = 0          # a locus nobody has a call at
    codes = np.ascontiguousarray(codes, np.uint32)
    called = codes != 0
    compared = called.astype(np.int64) @ called.astype(np.int64).T
    differ = ((codes[:, None, :] != codes[None, :, :]) & called[:, None, :] & called[None, :, :]).sum(-1)
    codes.setflags(write=False)
    return codes, differ.astype(np.uint32), compared.astype(np.uint32)


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_both_matrices_equal_numpy(hip_ctx, A, L, alleles, miss):
    import colorid_amd
    codes, differ, compared = table(A, L, alleles, miss)
    if alleles == "wide":
        assert codes.max() == 0xFFFFFFFD
    d = colorid_amd.Dists(hip_ctx, codes)
    got_d, got_c = d.rows()
    d.close()
    assert np.array_equal(got_c, compared)
    assert np.array_equal(got_d, differ)
    if A >= 3:
        assert not got_c[A - 1].any() and not got_d[A - 1].any()       # nothing is compared with the accession without a call
    if A >= 2:
        assert got_d[0, 1] == 0 and got_c[0, 1] == got_c[0, 0]         # identical accessions


@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_row_blocks(hip_ctx, A, L):
    import colorid_amd
    codes, differ, compared = table(A, L, "few", 0.3)
    d = colorid_amd.Dists(hip_ctx, codes)
    for row0, n in ((0, A), (1, 1), (63, 2), (64, 66), (A - 1, 1)):
        if row0 < 0 or row0 + n > A:
            continue
        got_d, got_c = d.rows(row0, n)
        assert np.array_equal(got_d, differ[row0:row0 + n]) and np.array_equal(got_c, compared[row0:row0 + n]), (row0, n)
        only_d, none = d.rows(row0, n, compared=False)                  # compared = NULL
        assert none is None and np.array_equal(only_d, differ[row0:row0 + n]), (row0, n)
    for row0 in (0, A):                                                 # n_rows = 0: a no-op
        got_d, got_c = d.rows(row0, 0)
        assert got_d.shape == (0, A) and got_c.shape == (0, A)
    # the matrix put together from blocks of 48 rows (no multiple of the tile): symmetric, nothing differs on the diagonal
    blocks = [d.rows(r, min(48, A - r)) for r in range(0, A, 48)]
    full_d, full_c = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    d.close()
    assert np.array_equal(full_d, differ) and np.array_equal(full_c, compared)
    assert np.array_equal(full_d, full_d.T) and np.array_equal(full_c, full_c.T) and not np.diagonal(full_d).any()
    assert np.array_equal(np.diagonal(full_c), (codes != 0).sum(1))


def test_slices_of_a_block_give_the_same_matrices(hip_ctx, tune):
    import colorid_amd
    codes, differ, compared = table(130, 100, "few", 0.3)
    tune("dense_report_bytes", 4096)        # 130 x 4 bytes a row and matrix: 3 rows a slice with compared, 7 without
    d = colorid_amd.Dists(hip_ctx, codes)
    got_d, got_c = d.rows()
    only_d, _ = d.rows(5, 120, compared=False)
    tune("dense_report_bytes", 1)           # less than one row: slices of one row
    one_d, one_c = d.rows(60, 9)
    d.close()
    assert np.array_equal(got_d, differ) and np.array_equal(got_c, compared)
    assert np.array_equal(only_d, differ[5:125])
    assert np.array_equal(one_d, differ[60:69]) and np.array_equal(one_c, compared[60:69])


@pytest.mark.parametrize("bad", [0xFFFFFFFE, 0xFFFFFFFF])
def test_reserved_codes_are_refused(hip_ctx, bad):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID
    codes = np.array(table(65, 33, "few", 0.3)[0])
    codes[64, 32] = bad                     # the last cell: the second tile of accessions, the second chunk of loci
    with pytest.raises(colorid_amd.CidError) as ei:
        colorid_amd.Dists(hip_ctx, codes)
    assert ei.value.code == CID_ERR_INVALID and "0xFFFFFFFE" in str(ei.value)
    codes[64, 32] = 0xFFFFFFFD              # the context is as good as before
    d = colorid_amd.Dists(hip_ctx, codes)
    assert d.rows(64, 1)[1][0, 64] == (codes[64] != 0).sum()
    d.close()


def test_shape_and_range_errors(hip_ctx):
    import colorid_amd
    from colorid_amd._lib import CID_ERR_INVALID, check
    for shape in ((0, 5), (5, 0), (0, 0)):  # n_acc = 0, n_loci = 0
        with pytest.raises(colorid_amd.CidError) as ei:
            colorid_amd.Dists(hip_ctx, np.zeros(shape, np.uint32))
        assert ei.value.code == CID_ERR_INVALID
    d = colorid_amd.Dists(hip_ctx, table(65, 33, "few", 0.3)[0])
    for row0, n in ((0, 66), (65, 1), (64, 2), (66, 0), (0xFFFFFFFF, 2)):   # row0 + n_rows > n_acc (the last: past 2^32)
        buf = np.zeros((max(n, 1), 65), np.uint32)
        with pytest.raises(colorid_amd.CidError) as ei:
            check(d.lib.cid_dists_rows(d.h, row0, n, buf.ctypes.data, buf.ctypes.data))
        assert ei.value.code == CID_ERR_INVALID, (row0, n)
    d.close()
