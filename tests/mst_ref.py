"""The reference of `dists --mst` (no test functions): the minimum spanning forest of a cgMLST table, in plain Python over numpy matrices.

Graph: the accessions 0 .. A - 1; {i, j}, i != j, is an edge iff compared(i, j) >= M.  Edge key, a strict total order: differ ascending,
then compared DESCENDING, then lo = min(i, j), then hi = max(i, j).  The forest is what Kruskal's algorithm gives over the edges sorted by
that key; the key being strict, it is the only minimum spanning forest there is.

    matrices(codes)            -> (differ, compared), the numpy formulas of test_gpu_dists.py
    forest(differ, compared,M) -> [(lo, hi, differ, compared)] in edge-key order
    nearest(differ, compared,M)-> per accession (j, differ, compared) or None: the `nearest` rule of clusters.tsv
    components(A, edges)       -> per accession the smallest member of its tree
    cut(A, edges, T)           -> components after dropping the edges with differ > T
    mst_tsv / mst_nwk          -> the text of PREFIX.mst.tsv / PREFIX.mst.nwk
"""
import numpy as np

NONE = 0xFFFFFFFF


def matrices(codes):
    codes = np.asarray(codes, np.uint32)
    called = codes != 0
    compared = called.astype(np.int64) @ called.astype(np.int64).T
    differ = ((codes[:, None, :] != codes[None, :, :]) & called[:, None, :] & called[None, :, :]).sum(-1)
    return differ.astype(np.int64), compared.astype(np.int64)


def edge_key(differ, compared, lo, hi):
    return (int(differ), -int(compared), int(lo), int(hi))


def all_edges(differ, compared, M):
    """every edge of the graph as (lo, hi, differ, compared), sorted by the edge key"""
    A = len(differ)
    M = max(int(M), 1)
    lo, hi = np.triu_indices(A, 1)
    keep = compared[lo, hi] >= M
    lo, hi = lo[keep], hi[keep]
    d, c = differ[lo, hi], compared[lo, hi]
    order = np.lexsort((hi, lo, -c, d))
    return [(int(lo[k]), int(hi[k]), int(d[k]), int(c[k])) for k in order]


class UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)      # the root is the smallest member
        return True


def forest(differ, compared, M=1):
    uf = UnionFind(len(differ))
    return [e for e in all_edges(differ, compared, M) if uf.union(e[0], e[1])]


def nearest(differ, compared, M=1, comp=None):
    """per accession i the j minimal in (differ, -compared, j) over j != i with compared >= M — with comp, over the j of another label"""
    A = len(differ)
    M = max(int(M), 1)
    out = []
    for i in range(A):
        best = None
        for j in range(A):
            if (j == i if comp is None else comp[j] == comp[i]) or compared[i, j] < M:
                continue
            k = (int(differ[i, j]), -int(compared[i, j]), j)
            if best is None or k < best:
                best = k
        out.append(None if best is None else (best[2], best[0], -best[1]))
    return out


def components(A, edges):
    uf = UnionFind(A)
    for e in edges:
        uf.union(e[0], e[1])
    return [uf.find(i) for i in range(A)]


def cut(A, edges, T):
    return components(A, [e for e in edges if e[2] <= T])


def linked(differ, compared, T, M=1):
    """the clusters of --cluster T --min-compared M: a plain union-find over all links"""
    A = len(differ)
    M = max(int(M), 1)
    uf = UnionFind(A)
    for i in range(A):
        for j in range(i + 1, A):
            if compared[i, j] >= M and differ[i, j] <= T:
                uf.union(i, j)
    return [uf.find(i) for i in range(A)]


def mst_tsv(names, edges):
    return "a\tb\tdiffer\tcompared\n" + "".join(f"{names[lo]}\t{names[hi]}\t{d}\t{c}\n" for lo, hi, d, c in edges)


def nwk_name(name):
    if name == "" or any(ch.isspace() or ch in "()[]':;," for ch in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def mst_nwk(names, edges):
    """one line per tree in order of its first member, rooted there; children in ascending table order; (child,..)name:differ"""
    A = len(names)
    adj = [[] for _ in range(A)]
    for lo, hi, d, _ in edges:
        adj[lo].append((hi, d))
        adj[hi].append((lo, d))
    for a in adj:
        a.sort()
    seen = [False] * A
    lines = []
    for root in range(A):
        if seen[root]:
            continue
        seen[root] = True
        out = []
        # frames: [node, length of the edge to its parent (None at the root), its children, the next child]
        stack = [[root, None, [x for x in adj[root]], 0]]
        while stack:
            f = stack[-1]
            node, length, kids, k = f
            if k == 0 and kids:
                out.append("(")
            if k < len(kids):
                if k:
                    out.append(",")
                f[3] += 1
                child, d = kids[k]
                seen[child] = True
                stack.append([child, d, [x for x in adj[child] if x[0] != node], 0])
                continue
            if kids:
                out.append(")")
            out.append(nwk_name(names[node]))
            if length is not None:
                out.append(f":{length}")
            stack.pop()
        lines.append("".join(out) + ";\n")
    return "".join(lines)


def summary(A, edges):
    """(trees, edges, total length): the numbers of the closing stderr line"""
    return A - len(edges), len(edges), sum(e[2] for e in edges)
