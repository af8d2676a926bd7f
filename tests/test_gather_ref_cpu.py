"""tests/gather_ref.py, the statement of the greedy cover the GPU tests compare against, on matrices small enough to work out by hand."""
import numpy as np

from gather_ref import gather


def P_of(cols, n):
    """cols: per colour the k-mers that have it"""
    P = np.zeros((n, len(cols)), bool)
    for c, ks in enumerate(cols):
        P[list(ks), c] = True
    return P


def brief(rows):
    return [(r["colour"], r["new_kmers"]) for r in rows]


def test_a_tie_goes_to_the_lower_index():
    P = P_of([{0, 1}, {2, 3}, {4}], 5)
    rows, n_hit, ties = gather(P)
    assert brief(rows) == [(0, 2), (1, 2), (2, 1)] and ties == [2, 1, 1] and n_hit == 5
    assert [r["live_before"] for r in rows] == [5, 3, 1]
    rows, _, _ = gather(P[:, ::-1])                  # the same sets, the colours reversed: still the lower index first
    assert brief(rows) == [(1, 2), (2, 2), (0, 1)]


def test_identical_columns_give_one_row():
    P = P_of([{0, 1, 2}, {5}, {0, 1, 2}], 6)
    rows, n_hit, ties = gather(P)
    assert brief(rows) == [(0, 3), (1, 1)] and ties[0] == 2 and n_hit == 4
    assert rows[0]["total_kmers"] == 3


def test_a_subset_of_the_first_pick_never_appears():
    P = P_of([{1, 2}, {0, 1, 2, 3}, {3, 4}], 6)
    rows, _, _ = gather(P)
    assert brief(rows) == [(1, 4), (2, 1)]
    assert rows[1]["total_kmers"] == 2 and rows[1]["live_before"] == 2        # k-mer 5 has no colour and stays live


def test_weights_follow_the_kmers_a_row_takes():
    P = P_of([{0, 1, 2}, {2, 3}], 4)
    rows, _, _ = gather(P, freq=[10, 20, 30, 40])
    assert rows[0] == dict(colour=0, new_kmers=3, new_weight=60, total_kmers=3, total_weight=60, live_before=4)
    assert rows[1] == dict(colour=1, new_kmers=1, new_weight=40, total_kmers=2, total_weight=70, live_before=1)
    rows, _, _ = gather(P)                           # no multiplicities: every k-mer weighs 1
    assert [(r["new_weight"], r["total_weight"]) for r in rows] == [(3, 3), (1, 2)]


def test_min_new_ends_the_cover():
    P = P_of([{0, 1, 2, 3}, {4, 5}, {6}], 7)
    assert brief(gather(P, min_new=1)[0]) == [(0, 4), (1, 2), (2, 1)]
    assert brief(gather(P, min_new=2)[0]) == [(0, 4), (1, 2)]
    assert brief(gather(P, min_new=3)[0]) == [(0, 4)]
    assert brief(gather(P, min_new=5)[0]) == []
    # new, not total, is what min_new looks at
    P = P_of([{0, 1, 2, 3}, {2, 3, 4}], 5)
    assert brief(gather(P, min_new=2)[0]) == [(0, 4)]


def test_max_rows_ends_the_cover():
    P = P_of([{0, 1, 2, 3}, {4, 5}, {6}], 7)
    assert brief(gather(P, max_rows=2)[0]) == [(0, 4), (1, 2)]
    assert gather(P, max_rows=0) == ([], 7, [])
    assert brief(gather(P, max_rows=100)[0]) == [(0, 4), (1, 2), (2, 1)]


def test_empty_input():
    assert gather(np.zeros((0, 5), bool)) == ([], 0, [])
    assert gather(np.zeros((0, 5), bool), freq=np.zeros(0, np.uint32)) == ([], 0, [])
    assert gather(np.zeros((3, 0), bool)) == ([], 0, [])


def test_all_zero_rows():
    assert gather(np.zeros((9, 4), bool), freq=np.arange(1, 10)) == ([], 0, [])
    P = np.zeros((9, 4), bool)
    P[4, 2] = True
    rows, n_hit, _ = gather(P, freq=np.arange(1, 10))
    assert rows == [dict(colour=2, new_kmers=1, new_weight=5, total_kmers=1, total_weight=5, live_before=9)] and n_hit == 1
