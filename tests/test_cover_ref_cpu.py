"""tests/cover_ref.py — the numpy restatement of the coverage search's definitions that the GPU tests compare against — on hand-written
masks whose answers are worked out here, field by field."""
import numpy as np

import cover_ref
from cover_ref import NONE

K = 5


def one(col, first=None, k=K):
    """the cell of a single colour as a plain tuple: kmers_hit, windows_hit, bases_covered, n_runs, longest_run, first_window, last_window, reserved"""
    col = np.asarray(col, bool)
    out = cover_ref.cover(col[:, None], first, k)
    assert out.shape == (1,) and out.dtype == cover_ref.DTYPE
    assert int(out["bases_covered"][0]) == cover_ref.bases_by_gaps(col, k)      # the union, counted base by base == the closed form
    return tuple(int(x) for x in out[0])


def mask(L, *ranges):
    m = np.zeros(L, bool)
    for a, b in ranges:
        m[a:b] = True
    return m


def test_empty_segment_and_segment_without_a_hit():
    assert one(np.zeros(0, bool)) == (0, 0, 0, 0, 0, NONE, NONE, 0)
    assert one(np.zeros(40, bool)) == (0, 0, 0, 0, 0, NONE, NONE, 0)
    assert cover_ref.cover(np.zeros((0, 3), bool), None, K).shape == (3,)


def test_a_single_window():
    # one window of k bases: it covers k bases, one run of one window, at window 0
    assert one([True]) == (1, 1, K, 1, 1, 0, 0, 0)
    # the same window at position 7 of 20
    assert one(mask(20, (7, 8))) == (1, 1, K, 1, 1, 7, 7, 0)


def test_all_ones_over_130_windows():
    # 130 windows in one run cover 130 + k - 1 bases
    assert one(np.ones(130, bool)) == (130, 130, 130 + K - 1, 1, 130, 0, 129, 0)
    assert one(np.ones(130, bool), k=31) == (130, 130, 160, 1, 130, 0, 129, 0)


def test_two_runs_around_a_gap_of_k_minus_2_k_minus_1_and_k():
    """runs of 10 and 6 windows.  The first run's last window covers bases up to 9 + k - 1 = 13 (k = 5); the second run starts at window
    10 + gap.  gap = k-2 = 3: second run starts at base 13, still overlapping -> every base from 0 to the end is covered.
    gap = k-1 = 4: it starts at base 14, the first base after the first run's reach -> still no hole.
    gap = k = 5: it starts at base 15 -> base 14 is the one uncovered base."""
    span = {}
    for gap in (K - 2, K - 1, K):
        L = 10 + gap + 6
        got = one(mask(L, (0, 10), (10 + gap, L)))
        total_bases = L + K - 1
        span[gap] = total_bases - got[2]          # uncovered bases of the record
        assert got[0] == got[1] == 16 and got[3:] == (2, 10, 0, L - 1, 0)
        assert got[2] == 16 + min(gap, K - 1) + K - 1
    assert span == {K - 2: 0, K - 1: 0, K: 1}


def test_a_run_that_ends_on_bit_63_and_goes_on_at_bit_64():
    # windows 60 .. 69 hit: ONE run of 10 across the boundary of two 64-window words, 10 + k - 1 bases
    assert one(mask(130, (60, 70))) == (10, 10, 10 + K - 1, 1, 10, 60, 69, 0)
    # ... and a run that ends exactly on bit 63, the next one starting on bit 65: two runs, gap 1
    assert one(mask(130, (50, 64), (65, 70))) == (19, 19, 19 + 1 + K - 1, 2, 14, 50, 69, 0)
    # a run over three words: 63 .. 128
    assert one(mask(130, (63, 129))) == (66, 66, 66 + K - 1, 1, 66, 63, 128, 0)


def test_invalid_windows_break_a_run():
    """20 windows whose k-mers are all in the colour; windows 8 and 9 contain an N and are invalid, so P is false there: two runs of 8 and
    10, gap 2 < k - 1: no base is uncovered by the definition (the union of the windows that hit)"""
    valid = np.ones(20, bool)
    valid[8:10] = False
    P = np.ones(20, bool) & valid
    assert one(P) == (18, 18, 18 + 2 + K - 1, 2, 10, 0, 19, 0)


def test_first_mask_only_changes_kmers_hit():
    # windows 12 .. 15 repeat the k-mers of windows 2 .. 5: they are no first occurrences
    col = mask(20, (0, 8), (12, 18))
    first = np.ones(20, bool)
    first[12:16] = False
    with_all = one(col)
    with_first = one(col, first)
    assert with_all[0] == 14 and with_first[0] == 10
    assert with_all[1:] == with_first[1:] == (14, 14 + 4 + K - 1, 2, 8, 0, 17, 0)


def test_many_colours_at_once_and_three_runs():
    L = 200
    P = np.zeros((L, 3), bool)
    P[:, 0] = mask(L, (5, 6), (50, 120), (199, 200))     # three runs, both gaps above k - 1
    P[:, 2] = True
    out = cover_ref.cover(P, None, 31)
    assert tuple(out[0]) == (72, 72, 72 + 3 * 30, 3, 70, 5, 199, 0)
    assert tuple(out[1]) == (0, 0, 0, 0, 0, NONE, NONE, 0)
    assert tuple(out[2]) == (200, 200, 230, 1, 200, 0, 199, 0)
