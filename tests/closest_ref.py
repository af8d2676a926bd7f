"""The reference of `dists --closest K` (no test functions): every accession's K nearest in plain Python loops, over the (differ, compared)
matrices that test_gpu_dists.table or test_gpu_cli_dists.matrices give.

The CANDIDATES of accession a are the b != a with compared[a][b] >= max(M, 1) and differ[a][b] <= T (T = None: no bound).  Their order:
differ ascending, then compared DESCENDING, then b ascending — strict for a fixed a, so the K nearest are unique.

    closest(differ, compared, K, T, M, rows)       -> per a of `rows` (a range; default all) a list of K tuples (a, b, differ, compared);
                                                      the ranks past the candidates are (a, NONE, 0, 0) — what cid_dists_closest returns
    closest_tsv(names, differ, compared, K, T, M)  -> the text of PREFIX.closest.tsv
    query_tsv_cut(names, D, differ, compared, K, T, M) -> the text of PREFIX.query.tsv under --closest K: within_ref.query_tsv's lines,
                                                      the first K of every query accession
"""
import within_ref

NONE = 0xFFFFFFFF
UNBOUNDED = 0xFFFFFFFF


def closest(differ, compared, K, T=None, M=1, rows=None):
    A = len(differ)
    M = max(int(M), 1)
    out = []
    for a in (range(A) if rows is None else rows):
        best = []                                     # the candidates seen so far, nearest first, never more than K: an insertion sort
        for b in range(A):
            if b == a or compared[a][b] < M or (T is not None and differ[a][b] > T):
                continue
            d, c = int(differ[a][b]), int(compared[a][b])
            at = len(best)
            while at > 0:
                _, pb, pd, pc = best[at - 1]
                if (pd, -pc, pb) < (d, -c, b):
                    break
                at -= 1
            best.insert(at, (a, b, d, c))
            del best[K:]
        out.append(best + [(a, NONE, 0, 0)] * (K - len(best)))
    return out


def closest_tsv(names, differ, compared, K, T=None, M=1):
    out = "accession\tneighbour\tdiffer\tcompared\n"
    for a, near in enumerate(closest(differ, compared, K, T, M)):
        if near[0][1] == NONE:
            out += f"{names[a]}\t-\t-\t-\n"
        for _, b, d, c in near:
            if b != NONE:
                out += f"{names[a]}\t{names[b]}\t{d}\t{c}\n"
    return out


def query_tsv_cut(names, D, differ, compared, K, T=None, M=1):
    """within_ref.query_tsv with every query accession's run of lines cut to its first K (T = None: a threshold no pair exceeds)"""
    bound = max((int(v) for row in differ for v in row), default=0) if T is None else T
    lines = within_ref.query_tsv(names, D, differ, compared, bound, M).split("\n")
    out, seen = [lines[0]], {}
    for line in lines[1:-1]:
        q = line.split("\t")[0]
        seen[q] = seen.get(q, 0) + 1
        if seen[q] <= K:
            out.append(line)
    return "\n".join(out) + "\n"
