"""tests/closest_ref.py, the reference of `dists --closest K`, against a numpy restatement (a stable lexsort per row) and against
within_ref.neighbours cut at K, over the tables of test_gpu_dists.py (no GPU); by hand on the table of tests/golden/alleles; and what
those tables exercise at M = 1 without a bound: rows where the ranks K and K + 1 tie in (differ, compared) so that only the column
decides, rows with fewer than K candidates, and rows whose K nearest come from more than one tile of 64 columns."""
import numpy as np
import pytest

import closest_ref
import within_ref
from test_gpu_cli_dists import GOLD, matrices, parse_table
from test_gpu_dists import table

SHAPES = [(1, 1), (2, 1), (3, 7), (63, 31), (64, 32), (65, 33), (130, 100), (257, 1), (200, 1025)]
INPUTS = [("few", 0.0), ("few", 0.3), ("wide", 0.3)]


def closest_np(differ, compared, K, T=None, M=1):
    """[A, K, 4] int64: per row the candidates ordered by one lexsort over (b, -compared, differ), the last key the most significant"""
    A = len(differ)
    d, c = np.asarray(differ, np.int64), np.asarray(compared, np.int64)
    out = np.zeros((A, K, 4), np.int64)
    out[:, :, 0] = np.arange(A)[:, None]
    out[:, :, 1] = closest_ref.NONE
    for a in range(A):
        ok = (c[a] >= max(M, 1)) & (np.arange(A) != a)
        if T is not None:
            ok &= d[a] <= T
        b = np.nonzero(ok)[0]
        b = b[np.lexsort((b, -c[a, b], d[a, b]))][:K]
        out[a, :len(b), 1], out[a, :len(b), 2], out[a, :len(b), 3] = b, d[a, b], c[a, b]
    return out


@pytest.mark.parametrize("alleles,miss", INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("A,L", SHAPES, ids=lambda v: str(v))
def test_the_reference_equals_numpy_and_the_neighbour_lists_cut(A, L, alleles, miss):
    _, differ, compared = table(A, L, alleles, miss)
    dl, cl = differ.tolist(), compared.tolist()
    for K in (1, 3, 64):
        for T in (2, None):
            for M in sorted({1, max(1, L // 2)}):
                got = closest_ref.closest(dl, cl, K, T, M)
                assert np.array_equal(np.array(got, np.int64).reshape(A, K, 4), closest_np(differ, compared, K, T, M)), (K, T, M)
                near = within_ref.neighbours(dl, cl, 0, L if T is None else T, M)
                for a in range(A):
                    assert [g[1:] for g in got[a] if g[1] != closest_ref.NONE] == near[a][:K], (K, T, M, a)
    rows = range(A // 2, A)
    assert closest_ref.closest(dl, cl, 3, None, 1, rows) == closest_ref.closest(dl, cl, 3)[A // 2:]
    assert closest_ref.closest(dl, cl, 3, None, 0) == closest_ref.closest(dl, cl, 3, None, 1)          # M = 0 is M = 1


def census(A, L, alleles, miss, K):
    """(rows where the ranks K and K + 1 tie in (differ, compared), rows with fewer than K candidates, rows whose K nearest lie in more
    than one column tile) at M = 1 without a bound"""
    _, differ, compared = table(A, L, alleles, miss)
    near = closest_np(differ, compared, min(K + 1, max(A, 1)))
    tie = short = spread = 0
    for a in range(A):
        b = near[a, :, 1]
        have = int((b != closest_ref.NONE).sum())
        short += have < K
        tie += have > K and tuple(near[a, K - 1, 2:]) == tuple(near[a, K, 2:])
        spread += len({int(x) // 64 for x in b[:min(have, K)]}) > 1
    return tie, short, spread


def test_what_the_tables_exercise():
    assert census(130, 100, "few", 0.0, 3)[0] == 64 and census(130, 100, "few", 0.0, 64)[0] == 116     # a tie at the cut
    assert census(257, 1, "few", 0.0, 3)[0] == 256 and census(257, 1, "few", 0.0, 64)[0] == 256
    for A, L in SHAPES:
        for alleles, miss in INPUTS:
            if A >= 3:
                assert census(A, L, alleles, miss, 1)[1] >= 1                                           # the accession without a call
    assert census(65, 33, "few", 0.0, 64)[1] == 65                                                      # 64 others at the most: every row is short
    assert census(130, 100, "few", 0.0, 3)[2] == 89                                                     # three from more than one tile
    for A, L in ((130, 100), (257, 1), (200, 1025)):
        tie, short, spread = census(A, L, "few", 0.0, 64)
        assert spread == A - 1, (A, L)                                                                  # all but the accession without a call
    _, differ, compared = table(130, 100, "few", 0.0)
    bounded = closest_ref.closest(differ.tolist(), compared.tolist(), 3, 2, 1)
    assert sum(1 for row in bounded if row[2][1] == closest_ref.NONE) > 120                             # with T = 2 almost every row is short


def test_by_hand_on_the_golden_table():
    accs, loci, cells = parse_table(open(GOLD).read())
    differ, compared = matrices(cells, len(loci))
    assert accs == ["acc_A", "acc_B", "acc_C", "acc_late", "sample 4"]
    # acc_A: B (0, 1) and late (0, 1) tie and the table's order decides, then C (1, 2) before `sample 4` (1, 1): more shared loci first
    assert closest_ref.closest_tsv(accs, differ, compared, 3).splitlines()[:4] == [
        "accession\tneighbour\tdiffer\tcompared", "acc_A\tacc_B\t0\t1", "acc_A\tacc_late\t0\t1", "acc_A\tacc_C\t1\t2"]
    two = closest_ref.closest_tsv(accs, differ, compared, 64, None, 2)
    assert two == "accession\tneighbour\tdiffer\tcompared\nacc_A\tacc_C\t1\t2\nacc_B\t-\t-\t-\nacc_C\tacc_A\t1\t2\nacc_late\t-\t-\t-\nsample 4\t-\t-\t-\n"
    one = closest_ref.closest_tsv(accs, differ, compared, 1, 0)
    assert one == ("accession\tneighbour\tdiffer\tcompared\nacc_A\tacc_B\t0\t1\nacc_B\tacc_A\t0\t1\nacc_C\tsample 4\t0\t1\n"
                   "acc_late\tacc_A\t0\t1\nsample 4\tacc_C\t0\t1\n")
    assert closest_ref.closest_tsv([], [], [], 3) == "accession\tneighbour\tdiffer\tcompared\n"


def test_the_query_file_cut():
    query = "\tlmo0001\tnovel\tabcZ\nnew_1\t2\t5\t12\nnew_2\tNA\t5\tNA\nnew_3\t2\t\t12\n"
    al = within_ref.align(open(GOLD).read(), query)
    differ, compared = matrices(al.cells, len(al.loci))
    assert closest_ref.query_tsv_cut(al.accs, 5, differ, compared, 2, 0) == (
        "query\tneighbour\tin\tdiffer\tcompared\nnew_1\tacc_C\ttable\t0\t2\nnew_1\tnew_3\tquery\t0\t2\nnew_2\t-\t-\t-\t-\n"
        "new_3\tacc_C\ttable\t0\t2\nnew_3\tnew_1\tquery\t0\t2\n")
    for K in (1, 3, 64):
        for T in (0, 1, None):
            want = "query\tneighbour\tin\tdiffer\tcompared\n"
            for a, near in zip(range(5, 8), closest_ref.closest(differ.tolist(), compared.tolist(), K, T, 1, range(5, 8))):
                if near[0][1] == closest_ref.NONE:
                    want += f"{al.accs[a]}\t-\t-\t-\t-\n"
                for _, b, d, c in near:
                    if b != closest_ref.NONE:
                        want += f"{al.accs[a]}\t{al.accs[b]}\t{'table' if b < 5 else 'query'}\t{d}\t{c}\n"
            assert closest_ref.query_tsv_cut(al.accs, 5, differ, compared, K, T) == want, (K, T)
