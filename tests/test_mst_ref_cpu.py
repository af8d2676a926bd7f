"""tests/mst_ref.py, the reference of `dists --mst`, against hand-worked tables and against independent formulations: Kruskal over the
sorted edges (the reference) equals a Borůvka simulation written from the definition; the forest cut at T has the components of a plain
union-find over all links; the first Borůvka round is the `nearest` rule of clusters.tsv.  No GPU."""
import numpy as np
import pytest

import mst_ref


def forest_of(codes, M=1):
    differ, compared = mst_ref.matrices(np.array(codes, np.uint32))
    return mst_ref.forest(differ, compared, M)


def test_a_tie_broken_by_compared():
    # A-B: the loci 0 1 2, differ at 2.  A-C: the loci 1 2, differ at 2.  B-C: the loci 1 2 3, differ at 3.  All differ by 1; C goes to B,
    # with which it shares 3 loci, not to the earlier A, with which it shares 2
    codes = [[1, 1, 1, 0],
             [1, 1, 2, 2],
             [0, 1, 2, 1]]
    edges = forest_of(codes)
    assert edges == [(0, 1, 1, 3), (1, 2, 1, 3)]
    names = ["A", "B", "C"]
    assert mst_ref.mst_tsv(names, edges) == "a\tb\tdiffer\tcompared\nA\tB\t1\t3\nB\tC\t1\t3\n"
    assert mst_ref.mst_nwk(names, edges) == "((C:1)B:1)A;\n"
    assert mst_ref.summary(3, edges) == (1, 2, 2)


def test_a_tie_broken_by_lo_then_hi():
    # three identical accessions and one a locus away: every pair shares both loci; (0,1) < (0,2) < (1,2) and (0,3) < (1,3) < (2,3)
    codes = [[1, 1], [1, 1], [1, 1], [1, 2]]
    edges = forest_of(codes)
    assert edges == [(0, 1, 0, 2), (0, 2, 0, 2), (0, 3, 1, 2)]
    names = ["A", "B", "C", "D"]
    assert mst_ref.mst_tsv(names, edges) == "a\tb\tdiffer\tcompared\nA\tB\t0\t2\nA\tC\t0\t2\nA\tD\t1\t2\n"
    assert mst_ref.mst_nwk(names, edges) == "(B:0,C:0,D:1)A;\n"


QUOTED = ["acc 1", "a'b", "x(y)", "p:q", "plain", "none"]
TWO_TREES = [[1, 1, 0],     # acc 1
             [1, 2, 0],     # a'b     one locus from acc 1 and from plain
             [0, 0, 1],     # x(y)    shares the last locus with p:q only
             [0, 0, 2],     # p:q
             [1, 1, 0],     # plain   = acc 1
             [0, 0, 0]]     # none    without a call


def test_two_trees_an_accession_without_a_call_and_names_that_need_quotes():
    edges = forest_of(TWO_TREES)
    assert edges == [(0, 4, 0, 2), (0, 1, 1, 2), (2, 3, 1, 1)]
    assert mst_ref.mst_tsv(QUOTED, edges) == "a\tb\tdiffer\tcompared\nacc 1\tplain\t0\t2\nacc 1\ta'b\t1\t2\nx(y)\tp:q\t1\t1\n"
    assert mst_ref.mst_nwk(QUOTED, edges) == "('a''b':1,plain:0)'acc 1';\n('p:q':1)'x(y)';\nnone;\n"
    assert mst_ref.summary(6, edges) == (3, 3, 2)
    assert mst_ref.components(6, edges) == [0, 0, 2, 2, 0, 5]
    assert mst_ref.cut(6, edges, 0) == [0, 1, 2, 3, 0, 5]
    # two shared loci asked for: x(y) - p:q is no edge any more
    edges = forest_of(TWO_TREES, 2)
    assert edges == [(0, 4, 0, 2), (0, 1, 1, 2)]
    assert mst_ref.mst_nwk(QUOTED, edges) == "('a''b':1,plain:0)'acc 1';\n'x(y)';\n'p:q';\nnone;\n"
    assert forest_of(TWO_TREES, 3) == []


def test_names():
    for bare in ("a", "acc_1", "a.b-c|d", "0"):
        assert mst_ref.nwk_name(bare) == bare
    assert mst_ref.nwk_name("") == "''"
    for name, want in (("a b", "'a b'"), ("a\tb", "'a\tb'"), ("a'b", "'a''b'"), ("''", "''''''"), ("x(y)", "'x(y)'"), ("x[1]", "'x[1]'"),
                       ("p:q", "'p:q'"), ("p;q", "'p;q'"), ("p,q", "'p,q'")):
        assert mst_ref.nwk_name(name) == want


def test_a_chain_and_no_accession():
    n = 3000                                          # deeper than Python's recursion limit: the writer keeps its own stack
    edges = [(i, i + 1, 1, 5) for i in range(n - 1)]
    names = [f"n{i}" for i in range(n)]
    text = mst_ref.mst_nwk(names, edges)
    assert text.startswith("(" * (n - 1) + f"n{n - 1}:1)n{n - 2}:1)") and text.endswith(")n1:1)n0;\n") and text.count("\n") == 1
    assert mst_ref.mst_nwk([], []) == "" and mst_ref.mst_tsv([], []) == "a\tb\tdiffer\tcompared\n"
    assert mst_ref.mst_nwk(["a", "b c"], []) == "a;\n'b c';\n"


def random_table(seed):
    rng = np.random.default_rng(seed)
    A, L = int(rng.integers(2, 26)), int(rng.integers(1, 9))
    codes = rng.integers(1, 4, size=(A, L)).astype(np.uint32)          # few alleles: ties everywhere
    codes[rng.random((A, L)) < rng.choice([0.0, 0.3, 0.7])] = 0
    return codes


def boruvka(differ, compared, M):
    """from the definition: every component takes its least edge to another component, all of them are added, until none is left"""
    A = len(differ)
    comp = list(range(A))
    chosen = set()
    rounds = 0
    while True:
        best = {}
        for i in range(A):
            for j in range(A):
                if comp[i] != comp[j] and compared[i, j] >= M:
                    e = mst_ref.edge_key(differ[i, j], compared[i, j], min(i, j), max(i, j))
                    if comp[i] not in best or e < best[comp[i]]:
                        best[comp[i]] = e
        if not best:
            break
        rounds += 1
        chosen |= set(best.values())
        comp = mst_ref.components(A, [(lo, hi, d, -c) for d, c, lo, hi in chosen])
    return sorted(chosen), rounds


@pytest.mark.parametrize("seed", range(40))
def test_kruskal_equals_boruvka_and_the_cut_equals_the_clusters(seed):
    codes = random_table(seed)
    A, L = codes.shape
    differ, compared = mst_ref.matrices(codes)
    for M in (1, 2, L):
        edges = mst_ref.forest(differ, compared, M)
        keys = [mst_ref.edge_key(d, c, lo, hi) for lo, hi, d, c in edges]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        want, rounds = boruvka(differ, compared, M)
        assert keys == want
        assert rounds <= max(A - 1, 1).bit_length()
        assert all(lo < hi and compared[lo, hi] >= M and differ[lo, hi] == d and compared[lo, hi] == c for lo, hi, d, c in edges)
        assert len(edges) == A - len(set(mst_ref.components(A, edges)))
        for T in sorted(set(differ.ravel().tolist())):
            assert mst_ref.cut(A, edges, T) == mst_ref.linked(differ, compared, T, M), (M, T)
        # round one: every accession's nearest comparable neighbour, and that edge is in the forest
        near = mst_ref.nearest(differ, compared, M)
        assert near == mst_ref.nearest(differ, compared, M, comp=list(range(A)))
        for i, nb in enumerate(near):
            cand = [(differ[i, j], -compared[i, j], j) for j in range(A) if j != i and compared[i, j] >= M]
            assert nb == (None if not cand else (min(cand)[2], min(cand)[0], -min(cand)[1]))
            if nb is not None:
                assert (min(i, nb[0]), max(i, nb[0]), nb[1], nb[2]) in edges
