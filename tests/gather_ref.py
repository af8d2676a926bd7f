"""The greedy cover of include/colorid_hip.h (cid_search_gather) in plain numpy: P[n_kmers, n_colors] bool says which colours the AND of
a k-mer's rows holds, freq[n_kmers] its multiplicity (None: 1 each).

Round t over the live k-mers: new[c] = live k-mers with colour c; the pick is the colour with the largest new, ties to the lowest index;
the cover ends, emitting nothing, when that count is below min_new or max_rows rows are out.  A row says what the pick adds (new_kmers,
new_weight = the multiplicities of those k-mers), what it holds of the whole query (total_kmers, total_weight) and how many k-mers were
live before it; the pick's k-mers then leave the live set."""
import numpy as np

FIELDS = ("colour", "new_kmers", "new_weight", "total_kmers", "total_weight", "live_before")


def gather(P, freq=None, min_new=1, max_rows=None):
    """-> (rows: list of dicts with FIELDS, n_hit, ties: per emitted row the number of colours that shared the largest count)"""
    P = np.asarray(P, bool)
    n, C = P.shape
    assert min_new >= 1
    f = np.ones(n, np.int64) if freq is None else np.asarray(freq).astype(np.int64)
    max_rows = C if max_rows is None else max_rows
    total = P.sum(axis=0, dtype=np.int64)
    total_weight = (P * f[:, None]).sum(axis=0, dtype=np.int64) if n else np.zeros(C, np.int64)
    n_hit = int(P.any(axis=1).sum())
    live = np.ones(n, bool)
    rows, ties = [], []
    while len(rows) < max_rows and C:
        new = P[live].sum(axis=0, dtype=np.int64)
        c = int(np.argmax(new))                      # the first of the largest: the lowest colour index
        if new[c] < min_new:
            break
        take = live & P[:, c]
        rows.append(dict(colour=c, new_kmers=int(new[c]), new_weight=int(f[take].sum()), total_kmers=int(total[c]),
                         total_weight=int(total_weight[c]), live_before=int(live.sum())))
        ties.append(int((new == new[c]).sum()))
        live &= ~take
    return rows, n_hit, ties
