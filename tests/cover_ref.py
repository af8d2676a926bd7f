"""The coverage search's definitions (include/colorid_hip.h: cid_cover) restated in numpy, the reference of the GPU tests.

A segment is one record of L windows numbered 0 .. L-1 in sequence order; window w covers bases [w, w + k).  P[w, c] is true when window
w holds a k-mer (an invalid window is absent for every colour) and colour c is set in the AND of the n_hash rows of that k-mer.
`first[w]` says that w is the first window of its segment holding its k-mer.  Per colour:

  kmers_hit      windows with P and first
  windows_hit    windows with P
  bases_covered  size of the union of [w, w + k) over the windows with P — counted here base by base (bases_by_gaps: the closed form)
  n_runs         maximal runs of consecutive windows with P
  longest_run    windows of the longest run
  first_window, last_window   lowest and highest w with P, NONE when there is none
  reserved       0
"""
import numpy as np

NONE = 0xFFFFFFFF
WIN_VALID, WIN_FIRST = 1, 2
FIELDS = ("kmers_hit", "windows_hit", "bases_covered", "n_runs", "longest_run", "first_window", "last_window", "reserved")
DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def runs_of(col):
    """[(start, length)] of the maximal runs of True in a 1-d bool array"""
    d = np.diff(np.concatenate(([0], col.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return list(zip(starts.tolist(), (ends - starts).tolist()))


def cover(P, first, k):
    """P: bool [L, C]; first: bool [L] or None (every window is a first); -> structured array [C] of DTYPE.  All colours at once."""
    P = np.asarray(P, bool)
    L, C = P.shape
    first = np.ones(L, bool) if first is None else np.asarray(first, bool)
    out = np.zeros(C, DTYPE)
    out["first_window"] = out["last_window"] = NONE
    if L == 0:
        return out
    out["kmers_hit"] = (P & first[:, None]).sum(axis=0)
    out["windows_hit"] = P.sum(axis=0)
    # base b of the record's L + k - 1 is covered iff one of the windows b - k + 1 .. b hit: sums over k rows of P padded with absent windows
    cs = np.zeros((L + 2 * (k - 1) + 1, C), np.int64)
    cs[k:k + L] = np.cumsum(P, axis=0)
    cs[k + L:] = cs[k + L - 1]
    out["bases_covered"] = ((cs[k:] - cs[:-k]) > 0).sum(axis=0)
    before = np.zeros_like(P)
    before[1:] = P[:-1]
    out["n_runs"] = (P & ~before).sum(axis=0)
    run = np.zeros(C, np.int64)      # windows of the run that ends at the row in hand
    longest = np.zeros(C, np.int64)
    for w in range(L):
        run = (run + 1) * P[w]
        np.maximum(longest, run, out=longest)
    out["longest_run"] = longest
    hit = P.any(axis=0)
    out["first_window"][hit] = P.argmax(axis=0)[hit]
    out["last_window"][hit] = (L - 1 - P[::-1].argmax(axis=0))[hit]
    return out


def bases_by_gaps(col, k):
    """the closed form of bases_covered: windows_hit + sum over interior gaps of min(gap, k - 1) + (k - 1 if any window hit)"""
    runs = runs_of(np.asarray(col, bool))
    if not runs:
        return 0
    gaps = [runs[i + 1][0] - (runs[i][0] + runs[i][1]) for i in range(len(runs) - 1)]
    return sum(n for _, n in runs) + sum(min(g, k - 1) for g in gaps) + k - 1
