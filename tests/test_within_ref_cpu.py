"""tests/within_ref.py, the reference of `dists --within` and `dists --query`, checked by hand on the table of tests/golden/alleles (no GPU).
Rows: acc_A, acc_B, acc_C, acc_late, `sample 4`.  Shared loci: A-B lmo0001 (1 / 1), A-C abcZ (12 / 12) and lmo0001 (1 / 2), A-late Zlocus
(2 / 2), A-s4 lmo0001 (1 / 2), B-C lmo0001 (1 / 2), B-late lmo1000 (105 / 9), B-s4 lmo0001 (1 / 2), C-s4 lmo0001 (2 / 2); C-late and
late-s4 share nothing."""
import os

import within_ref
from test_gpu_cli_dists import GOLD, matrices, parse_table

NAMES = ["acc_A", "acc_B", "acc_C", "acc_late", "sample 4"]
QUERY = "\tlmo0001\tnovel\tabcZ\nnew_1\t2\t5\t12\nnew_2\tNA\t5\tNA\nnew_3\t2\t\t12\n"


def golden():
    accs, loci, cells = parse_table(open(GOLD).read())
    assert accs == NAMES and os.path.basename(GOLD) == "expected.raw.tsv"
    return accs, matrices(cells, len(loci))


def named(prs):
    return [(NAMES[a], NAMES[b], d, c) for a, b, d, c in prs]


def test_within_0_and_1_and_min_compared():
    accs, (differ, compared) = golden()
    assert named(within_ref.pairs(differ, compared, 0, 1)) == [("acc_A", "acc_B", 0, 1), ("acc_A", "acc_late", 0, 1), ("acc_C", "sample 4", 0, 1)]
    eight = [("acc_A", "acc_B", 0, 1), ("acc_A", "acc_C", 1, 2), ("acc_A", "acc_late", 0, 1), ("acc_A", "sample 4", 1, 1),
             ("acc_B", "acc_C", 1, 1), ("acc_B", "acc_late", 1, 1), ("acc_B", "sample 4", 1, 1), ("acc_C", "sample 4", 0, 1)]
    assert named(within_ref.pairs(differ, compared, 1, 1)) == eight
    for T in (0, 1, 6, 1000):                                 # no locus in common: never a pair, whatever T
        got = named(within_ref.pairs(differ, compared, T, 1))
        assert ("acc_C", "acc_late") not in [g[:2] for g in got] and ("acc_late", "sample 4") not in [g[:2] for g in got]
    assert named(within_ref.pairs(differ, compared, 1000, 0)) == eight      # M = 0 is M = 1
    assert named(within_ref.pairs(differ, compared, 1, 2)) == [("acc_A", "acc_C", 1, 2)]
    assert within_ref.within_tsv(accs, within_ref.pairs(differ, compared, 0, 1)) == (
        "a\tb\tdiffer\tcompared\nacc_A\tacc_B\t0\t1\nacc_A\tacc_late\t0\t1\nacc_C\tsample 4\t0\t1\n")


def test_full_mode_and_row_ranges():
    accs, (differ, compared) = golden()
    up = within_ref.pairs(differ, compared, 1, 1)
    full = within_ref.pairs(differ, compared, 1, 1, upper=False)
    assert full == sorted(up + [(b, a, d, c) for a, b, d, c in up]) and len(full) == 16
    assert within_ref.pairs(differ, compared, 1, 1, rows=range(2, 4), upper=False) == [p for p in full if 2 <= p[0] < 4]
    assert within_ref.pairs(differ, compared, 1, 1, rows=range(2, 4)) == [p for p in up if 2 <= p[0] < 4]
    assert within_ref.components(5, within_ref.pairs(differ, compared, 0, 1)) == [0, 0, 2, 0, 2]


def test_the_query_by_hand():
    al = within_ref.align(open(GOLD).read(), QUERY)
    assert al.accs == NAMES + ["new_1", "new_2", "new_3"] and al.D == 5
    assert al.loci == ["Zlocus", "abcZ", "lmo0001", "lmo0002", "lmo0010", "lmo1000"]
    assert (al.common, al.only_table, al.only_query) == (2, 4, 1)
    assert al.cells[5] == [None, "12", "2", None, None, None] and al.cells[6] == [None] * 6 and al.cells[7] == al.cells[5]
    differ, compared = matrices(al.cells, 6)
    want0 = ("query\tneighbour\tin\tdiffer\tcompared\n"
             "new_1\tacc_C\ttable\t0\t2\nnew_1\tnew_3\tquery\t0\t2\nnew_1\tsample 4\ttable\t0\t1\n"
             "new_2\t-\t-\t-\t-\n"
             "new_3\tacc_C\ttable\t0\t2\nnew_3\tnew_1\tquery\t0\t2\nnew_3\tsample 4\ttable\t0\t1\n")
    assert within_ref.query_tsv(al.accs, 5, differ, compared, 0, 1) == want0
    one = within_ref.query_tsv(al.accs, 5, differ, compared, 1, 1).splitlines()
    assert one[1:6] == ["new_1\tacc_C\ttable\t0\t2", "new_1\tnew_3\tquery\t0\t2", "new_1\tsample 4\ttable\t0\t1", "new_1\tacc_A\ttable\t1\t2",
                        "new_1\tacc_B\ttable\t1\t1"]
    assert one[6] == "new_2\t-\t-\t-\t-" and len(one) == 12
    # the aligned table as text reads back as itself
    assert within_ref.parse(within_ref.table_text(al.accs, al.loci, al.cells)) == (al.accs, al.loci, al.cells)
