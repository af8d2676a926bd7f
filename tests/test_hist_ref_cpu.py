"""tests/hist_ref.py, the reference of `dists --hist` and `dists --levels`, against itself and against the older references (no GPU): the
plain loops and the numpy form of both histograms agree on a few small tables, row ranges and modes; the sums say what the header
promises; the levels' columns are the clusters of mst_ref.linked and of test_gpu_cli_dists.clusters_text per threshold, and they nest;
by hand on the table of tests/golden/alleles (its pairs are listed in test_within_ref_cpu.py)."""
import numpy as np
import pytest

import hist_ref
import mst_ref
import within_ref
from test_gpu_cli_dists import GOLD, clusters_text, generated_table, matrices, parse_table


def small(A, L, seed, miss):
    rng = np.random.default_rng([A, L, seed])
    codes = rng.integers(1, 4, size=(A, L), dtype=np.uint32)
    codes[rng.random((A, L)) < miss] = 0
    if A >= 2:
        codes[1] = codes[0]
    if A >= 3:
        codes[A - 1] = 0
    return mst_ref.matrices(codes)


@pytest.mark.parametrize("A,L,miss", [(1, 1, 0.0), (2, 3, 0.0), (7, 5, 0.3), (20, 9, 0.3), (33, 70, 0.1)])
def test_the_loops_and_numpy_agree(A, L, miss):
    differ, compared = small(A, L, 1, miss)
    for M in sorted({0, 1, max(1, L // 2), L + 1}):
        for upper in (True, False):
            for row0, n in ((0, None), (0, 0), (A // 2, A - A // 2), (A - 1, 1), (A, 0)):
                dl, cl = hist_ref.hist_loops(differ, compared, L, M, row0, n, upper)
                dn, cn = hist_ref.hist_numpy(differ, compared, L, M, row0, n, upper)
                assert dn.dtype == cn.dtype == np.uint64 and dn.shape == cn.shape == (L + 1,)
                assert dn.tolist() == dl and cn.tolist() == cl, (M, upper, row0, n)
                rows = A - row0 if n is None else n
                pairs = sum(A - 1 - a for a in range(row0, row0 + rows)) if upper else rows * (A - 1)
                assert sum(cl) == pairs and sum(dl) == sum(cl[max(M, 1):])
                for T in (0, 2, L):
                    assert sum(dl[:T + 1]) == len(within_ref.pairs(differ, compared, T, M, range(row0, row0 + rows), upper))
    full, up = hist_ref.hist_loops(differ, compared, L), hist_ref.hist_loops(differ, compared, L, upper=True)
    assert full[0] == [2 * v for v in up[0]] and full[1] == [2 * v for v in up[1]]          # the matrices are symmetric


def test_the_golden_table_by_hand():
    accs, loci, cells = parse_table(open(GOLD).read())
    differ, compared = matrices(cells, len(loci))
    # ten pairs: C-late and late-s4 share nothing, A-C shares two loci (differ 1), the other seven one locus (three equal, four not)
    assert hist_ref.hist_loops(differ, compared, 6, upper=True) == ([3, 5, 0, 0, 0, 0, 0], [2, 7, 1, 0, 0, 0, 0])
    assert hist_ref.hist_loops(differ, compared, 6, 2, upper=True) == ([0, 1, 0, 0, 0, 0, 0], [2, 7, 1, 0, 0, 0, 0])
    assert hist_ref.hist_tsv(differ, compared, 6) == ("loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n"
                                                     "0\t3\t3\t2\n1\t5\t8\t7\n2\t0\t8\t1\n3\t0\t8\t0\n4\t0\t8\t0\n5\t0\t8\t0\n6\t0\t8\t0\n")
    assert hist_ref.hist_tsv([], [], 2) == "loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n0\t0\t0\t0\n1\t0\t0\t0\n2\t0\t0\t0\n"
    # the levels: at 0 {A, B, late} and {C, s4}; at 1 everything
    assert hist_ref.levels(differ, compared, [0, 1]) == {0: [1, 1, 2, 1, 2], 1: [1, 1, 1, 1, 1]}
    assert hist_ref.levels_tsv(accs, differ, compared, [0, 1]) == (
        "accession\tT1\tT0\taddress\nacc_A\t1\t1\t1.1\nacc_B\t1\t1\t1.1\nacc_C\t1\t2\t1.2\nacc_late\t1\t1\t1.1\nsample 4\t1\t2\t1.2\n")
    assert hist_ref.levels(differ, compared, [5], 2) == {5: [1, 2, 1, 3, 4]}                  # at least two shared loci: A-C alone


def numbered(roots):
    number = {}
    return [number.setdefault(r, len(number) + 1) for r in roots]


def test_the_levels_are_the_clusters_and_nest():
    text, accs = generated_table()
    _, loci, cells = parse_table(text)
    differ, compared = matrices(cells, len(loci))
    for M in (1, 20):
        thresholds = [7, 0, 2, 12, 40]
        lv = hist_ref.levels(differ, compared, thresholds, M)
        for t in thresholds:
            assert lv[t] == numbered(mst_ref.linked(differ, compared, t, M))
            file_text, _, _ = clusters_text(accs, differ, compared, t, M)
            assert [str(x) for x in lv[t]] == [l.split("\t")[1] for l in file_text.splitlines()[1:]]
            assert lv[t][0] == 1 and sorted(set(lv[t])) == list(range(1, max(lv[t]) + 1))
        order = sorted(thresholds)
        for fine, coarse in zip(order, order[1:]):             # nested: a finer cluster lies in one coarser cluster
            inside = {}
            for f, c in zip(lv[fine], lv[coarse]):
                assert inside.setdefault(f, c) == c
            assert max(lv[coarse]) <= max(lv[fine])
        assert max(lv[0]) > max(lv[40])
        lines = hist_ref.levels_tsv(accs, differ, compared, [7, 0, 2], M).splitlines()
        assert lines[0] == "accession\tT7\tT2\tT0\taddress" and len(lines) == 71
        for i, line in enumerate(lines[1:]):
            f = line.split("\t")
            assert f[0] == accs[i] and f[1:4] == [str(lv[7][i]), str(lv[2][i]), str(lv[0][i])] and f[4] == ".".join(f[1:4])
