"""The reference of `dists --within T` and `dists --query` (no test functions): neighbour lists of a cgMLST table in plain Python, over the
(differ, compared) matrices that test_gpu_cli_dists.matrices derives from a table's text (or test_gpu_dists.table from codes).

A pair (a, b), a != b, is WITHIN when compared[a][b] >= max(M, 1) and differ[a][b] <= T.

    pairs(differ, compared, T, M, rows, upper) -> [(a, b, differ, compared)] sorted by (a, b): a over `rows` (a range; default all),
                                                  b over all accessions, with upper only b > a — what cid_dists_within returns
    within_tsv(names, pairs)                   -> the text of PREFIX.within.tsv (pairs in upper mode over all rows)
    parse(text)                                -> (accessions, loci, cells) of a table's text, None where it says NA or nothing
    align(table_text, query_text)              -> Aligned: the query's accessions on the TABLE's loci, matched by name, below the table's
    neighbours(differ, compared, D, T, M)      -> per query accession (rows D ..) its neighbours [(b, differ, compared)], nearest first
    query_tsv(names, D, differ, compared, T, M)-> the text of PREFIX.query.tsv
"""
import collections


def pairs(differ, compared, T, M=1, rows=None, upper=True):
    A = len(differ)
    M = max(int(M), 1)
    out = []
    for a in (range(A) if rows is None else rows):
        for b in range(a + 1 if upper else 0, A):
            if b != a and compared[a][b] >= M and differ[a][b] <= T:
                out.append((a, b, int(differ[a][b]), int(compared[a][b])))
    return out


def within_tsv(names, prs):
    return "a\tb\tdiffer\tcompared\n" + "".join(f"{names[a]}\t{names[b]}\t{d}\t{c}\n" for a, b, d, c in prs)


def parse(text):
    lines = text.split("\n")
    head = lines[0].split("\t")
    assert head[0] == ""
    loci = [] if head[1:] == [""] else head[1:]
    accs, cells = [], []
    for line in lines[1:]:
        if line == "":
            continue
        f = line.split("\t")
        assert len(f) == len(loci) + 1
        accs.append(f[0])
        cells.append([None if c in ("NA", "") else c for c in f[1:]])
    return accs, loci, cells


Aligned = collections.namedtuple("Aligned", "accs loci cells D common only_table only_query")


def align(table_text, query_text):
    """the loci are the table's, in its order; a query locus the table lacks is ignored, a table locus the query lacks is no call"""
    t_accs, t_loci, t_cells = parse(table_text)
    q_accs, q_loci, q_cells = parse(query_text)
    assert len(set(t_loci)) == len(t_loci) and len(set(q_loci)) == len(q_loci) and not set(t_accs) & set(q_accs)
    col = {name: k for k, name in enumerate(q_loci)}
    cells = [list(r) for r in t_cells]
    for r in q_cells:
        cells.append([r[col[name]] if name in col else None for name in t_loci])
    common = sum(1 for name in t_loci if name in col)
    return Aligned(t_accs + q_accs, t_loci, cells, len(t_accs), common, len(t_loci) - common, len(q_loci) - common)


def table_text(accs, loci, cells):
    """a table's text from cells (None -> NA): the aligned and concatenated table as `dists -t` reads it"""
    head = "\t" + "\t".join(loci) + "\n" if loci else "\t\n"
    return head + "".join("\t".join([accs[a]] + ["NA" if c is None else c for c in cells[a]]) + "\n" for a in range(len(accs)))


def neighbours(differ, compared, D, T, M=1):
    A = len(differ)
    M = max(int(M), 1)
    out = []
    for a in range(D, A):
        cand = [(int(differ[a][b]), -int(compared[a][b]), b) for b in range(A) if b != a and compared[a][b] >= M and differ[a][b] <= T]
        out.append([(b, d, -c) for d, c, b in sorted(cand)])      # rows below D are the table's: table before query, each in file order
    return out


def query_tsv(names, D, differ, compared, T, M=1):
    out = "query\tneighbour\tin\tdiffer\tcompared\n"
    for k, near in enumerate(neighbours(differ, compared, D, T, M)):
        if not near:
            out += f"{names[D + k]}\t-\t-\t-\t-\n"
        for b, d, c in near:
            out += f"{names[D + k]}\t{names[b]}\t{'table' if b < D else 'query'}\t{d}\t{c}\n"
    return out


def components(A, prs):
    """per accession the smallest member of its connected component under the pairs"""
    parent = list(range(A))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for p in prs:
        a, b = find(p[0]), find(p[1])
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(A)]
