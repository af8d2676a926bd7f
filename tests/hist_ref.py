"""The reference of `dists --hist` and `dists --levels` (no test functions), over the (differ, compared) matrices that
test_gpu_dists.table, mst_ref.matrices or test_gpu_cli_dists.matrices give.

A pair (a, b) is COUNTED when a is one of the rows asked for, b != a and — upper — b > a.  Every counted pair adds 1 to
compared_hist[compared[a][b]]; those with compared[a][b] >= max(M, 1) add 1 to differ_hist[differ[a][b]].  Bins 0 .. L.

    hist_loops(differ, compared, L, M, row0, n, upper) -> (differ_hist, compared_hist), lists of L + 1 ints, by plain loops
    hist_numpy(differ, compared, L, M, row0, n, upper) -> the same as uint64 arrays, by np.bincount over the masked matrices
    hist_tsv(differ, compared, L, M)                   -> the text of PREFIX.hist.tsv (upper mode over all rows)
    levels(differ, compared, thresholds, M)            -> {t: [cluster number per accession]}: per threshold a union-find over ALL pairs
                                                          with compared >= M and differ <= t (no forest), numbered from 1 in order of
                                                          the first member — the `cluster` column of PREFIX.clusters.tsv at --cluster t
    levels_tsv(names, differ, compared, thresholds, M) -> the text of PREFIX.levels.tsv: the columns coarse to fine, then the address
"""
import numpy as np


def hist_loops(differ, compared, L, M=1, row0=0, n=None, upper=False):
    A = len(differ)
    n = A - row0 if n is None else n
    M = max(int(M), 1)
    dh, ch = [0] * (L + 1), [0] * (L + 1)
    for a in range(row0, row0 + n):
        for b in range(a + 1 if upper else 0, A):
            if b == a:
                continue
            ch[int(compared[a][b])] += 1
            if compared[a][b] >= M:
                dh[int(differ[a][b])] += 1
    return dh, ch


def hist_numpy(differ, compared, L, M=1, row0=0, n=None, upper=False):
    A = len(differ)
    n = A - row0 if n is None else n
    M = max(int(M), 1)
    d, c = np.asarray(differ)[row0:row0 + n].astype(np.int64), np.asarray(compared)[row0:row0 + n].astype(np.int64)
    rows, cols = np.arange(row0, row0 + n)[:, None], np.arange(A)[None, :]
    counted = (cols > rows) if upper else (cols != rows)
    ch = np.bincount(c[counted], minlength=L + 1)
    dh = np.bincount(d[counted & (c >= M)], minlength=L + 1)
    return dh.astype(np.uint64), ch.astype(np.uint64)


def hist_tsv(differ, compared, L, M=1):
    dh, ch = hist_numpy(differ, compared, L, M, upper=True) if len(differ) else ([0] * (L + 1), [0] * (L + 1))
    out, total = "loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n", 0
    for k in range(L + 1):
        total += int(dh[k])
        out += f"{k}\t{int(dh[k])}\t{total}\t{int(ch[k])}\n"
    return out


def levels(differ, compared, thresholds, M=1):
    A = len(differ)
    M = max(int(M), 1)
    out = {}
    for t in thresholds:
        parent = list(range(A))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for i in range(A):
            for j in range(i + 1, A):
                if compared[i][j] >= M and differ[i][j] <= t:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        number = {}
        out[t] = [number.setdefault(find(i), len(number) + 1) for i in range(A)]
    return out


def levels_tsv(names, differ, compared, thresholds, M=1):
    order = sorted(thresholds, reverse=True)
    lv = levels(differ, compared, order, M)
    out = "accession" + "".join(f"\tT{t}" for t in order) + "\taddress\n"
    for i, name in enumerate(names):
        numbers = [str(lv[t][i]) for t in order]
        out += name + "".join("\t" + x for x in numbers) + "\t" + ".".join(numbers) + "\n"
    return out
