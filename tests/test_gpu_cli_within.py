"""`colorid dists --within T [--min-compared M] [--no-matrices]`, `search -s -m --alleles PREFIX --dists --within T` and `colorid dists
--query TABLE2 --within T` end to end: PREFIX.within.tsv and PREFIX.query.tsv against tests/within_ref.py over matrices derived from the
tables' text, the other files against a run without --within, the pairs' components against clusters.tsv, the forest's edges of at most
T among the pairs, the stderr lines.  The table of tests/golden/alleles, the generated 70 x 40 table of test_gpu_cli_dists.py — whole, and
split into 60 database and 10 query accessions with the query's columns permuted, one locus dropped and a foreign one added."""
import os
import subprocess

import numpy as np
import pytest

import within_ref
from test_gpu_cli_alleles import BIN, run
from test_gpu_cli_alleles import env  # noqa: F401  (the module-scoped fixture: the four-phage index and its scheme)
from test_gpu_cli_dists import GOLD, generated_table, matrices, parse_table
from test_gpu_cli_mst import clusters_of, same_partition

pytestmark = pytest.mark.gpu

EXTS = ("dists.tsv", "compared.tsv", "clusters.tsv", "mst.tsv", "mst.nwk", "within.tsv", "query.tsv")
QUERY = "\tlmo0001\tnovel\tabcZ\nnew_1\t2\t5\t12\nnew_2\tNA\t5\tNA\nnew_3\t2\t\t12\n"


def read_files(prefix):
    return {ext: open(f"{prefix}.{ext}").read() for ext in EXTS if os.path.exists(f"{prefix}.{ext}")}


def dists_lines(err):
    return [l for l in err.splitlines() if l.startswith("dists: ")]


def within_line(prefix, n, T, M):
    return f"dists: {n} pairs within {T} differing loci (at least {M} shared), written to {prefix}.within.tsv"


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_within")
    text, _ = generated_table()
    (d / "gen.tsv").write_text(text)
    return d, {"gold": (GOLD, open(GOLD).read()), "gen": (str(d / "gen.tsv"), text)}


@pytest.mark.parametrize("which,T,M", [("gold", 0, 1), ("gold", 1, 2), ("gold", 3, 1), ("gold", 3, 20), ("gold", 40, 1),
                                       ("gen", 0, 1), ("gen", 3, 1), ("gen", 3, 20), ("gen", 40, 1)])
def test_within_file_and_the_files_beside_it(tables, which, T, M):
    d, t = tables
    path, text = t[which]
    extra = ["--min-compared", str(M)] if M != 1 else []
    plain, with_w, bare = (str(d / f"{which}{T}_{M}{k}") for k in "pwb")
    run("dists", "-t", path, "-o", plain, "--cluster", str(T), "--mst", *extra)
    out, err = run("dists", "-t", path, "-o", with_w, "--cluster", str(T), "--mst", "--within", str(T), *extra)
    accs, loci, cells = parse_table(text)
    differ, compared = matrices(cells, len(loci))
    prs = within_ref.pairs(differ, compared, T, M)
    want = within_ref.within_tsv(accs, prs)
    got = read_files(with_w)
    assert sorted(got) == sorted(EXTS[:6])
    assert got["within.tsv"] == want
    before = read_files(plain)
    assert sorted(before) == sorted(EXTS[:5]) and all(got[k] == before[k] for k in before)     # byte for byte
    # matrices line, within line, clusters line, forest line
    lines = dists_lines(err)
    assert len(lines) == 4 and lines[0].endswith(f"written to {with_w}.dists.tsv, {with_w}.compared.tsv")
    assert lines[1] == within_line(with_w, len(prs), T, M)
    assert " clusters of 2 or more at <= " in lines[2] and lines[3].startswith("dists: minimum spanning forest: ")
    # the components of the pairs are the clusters; every forest edge of at most T is a line of the file
    assert same_partition(clusters_of(got["clusters.tsv"]), within_ref.components(len(accs), prs))
    file_lines = set(got["within.tsv"].splitlines()[1:])
    edges = [l for l in got["mst.tsv"].splitlines()[1:] if int(l.split("\t")[2]) <= T]
    assert all(e in file_lines for e in edges) and (edges or not prs)
    # it is the matrices' cells above the diagonal with differ <= T and compared >= M, nothing else
    A = len(accs)
    cells_above = {(i, j) for i in range(A) for j in range(i + 1, A) if differ[i][j] <= T and compared[i][j] >= M}
    assert {(a, b) for a, b, _, _ in prs} == cells_above
    if which == "gen":
        assert not any({a, b} in ({0, 1}, {2, 3}) for a, b, _, _ in prs)                       # no locus in common: never a pair
    # --no-matrices --within T: that one file, the same bytes
    out, err = run("dists", "-t", path, "-o", bare, "--no-matrices", "--within", str(T), *extra)
    assert read_files(bare) == {"within.tsv": want}
    assert dists_lines(err) == [f"dists: {A} accessions x {len(loci)} loci, matrices not written (--no-matrices)", within_line(bare, len(prs), T, M)]


def test_a_run_without_within_says_what_it_said(tables):
    d, t = tables
    out, err = run("dists", "-t", GOLD, "-o", str(d / "quiet"), "--cluster", "1")
    assert len(dists_lines(err)) == 2 and "pairs within" not in err and sorted(read_files(d / "quiet")) == ["clusters.tsv", "compared.tsv", "dists.tsv"]


def test_search_dists_within_writes_what_dists_writes_from_the_raw_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "sw"), "--dists", "--within", "0")
    run("dists", "-t", str(d / "sw.raw.tsv"), "-o", str(d / "sw_again"), "--within", "0")
    got = read_files(d / "sw")
    assert sorted(got) == ["compared.tsv", "dists.tsv", "within.tsv"] and got == read_files(d / "sw_again")
    # Listeria_phage_B051 and Listeria_phage_B545 share locB_4: the one pair with a common call
    assert got["within.tsv"] == "a\tb\tdiffer\tcompared\nListeria_phage_B051\tListeria_phage_B545\t0\t1\n"
    assert dists_lines(err)[-1] == within_line(str(d / "sw"), 1, 0, 1)


def query_line(prefix, Q, D, al, table, query, n, T, M, none):
    return (f"dists: {Q} query accessions against {D}, {al.common} loci in common ({al.only_table} only in {table}, {al.only_query} only in "
            f"{query}); {n} neighbours within {T} differing loci (at least {M} shared), {none} queries without one, written to {prefix}.query.tsv")


@pytest.mark.parametrize("T", [0, 1])
def test_the_query_by_hand(tmp_path, T):
    (tmp_path / "new.tsv").write_text(QUERY)
    prefix = str(tmp_path / "q")
    out, err = run("dists", "-t", GOLD, "--query", str(tmp_path / "new.tsv"), "-o", prefix, "--within", str(T))
    got = read_files(prefix)
    assert sorted(got) == ["query.tsv"]
    al = within_ref.align(open(GOLD).read(), QUERY)
    differ, compared = matrices(al.cells, len(al.loci))
    assert got["query.tsv"] == within_ref.query_tsv(al.accs, al.D, differ, compared, T)
    lines = got["query.tsv"].splitlines()
    assert lines[1:4] == ["new_1\tacc_C\ttable\t0\t2", "new_1\tnew_3\tquery\t0\t2", "new_1\tsample 4\ttable\t0\t1"]
    if T == 0:
        assert lines[4:] == ["new_2\t-\t-\t-\t-", "new_3\tacc_C\ttable\t0\t2", "new_3\tnew_1\tquery\t0\t2", "new_3\tsample 4\ttable\t0\t1"]
    else:
        assert lines[4:7] == ["new_1\tacc_A\ttable\t1\t2", "new_1\tacc_B\ttable\t1\t1", "new_2\t-\t-\t-\t-"]
    assert (al.common, al.only_table, al.only_query) == (2, 4, 1)
    n = len([l for l in lines[1:] if not l.endswith("\t-")])
    assert dists_lines(err) == [query_line(prefix, 3, 5, al, GOLD, str(tmp_path / "new.tsv"), n, T, 1, 1)]


def split_generated():
    """the generated table as 60 database and 10 query accessions — three of the near copies of accession 9 and the last seven are the
    query — the query's columns permuted, loc007 dropped, a foreign locus added"""
    text, accs = generated_table()
    lines = text.split("\n")
    asked = [12, 13, 14] + list(range(63, 70))
    db = "\n".join(l for k, l in enumerate(lines[:71]) if k - 1 not in asked) + "\n"
    loci = lines[0].split("\t")[1:]
    order = [int(k) for k in np.random.default_rng(7).permutation(len(loci)) if loci[int(k)] != "loc007"]
    rows = [lines[1 + a].split("\t") for a in asked]
    foreign_at = 5
    head = [loci[k] for k in order]
    head.insert(foreign_at, "elsewhere")
    q = "\t" + "\t".join(head) + "\n"
    for r in rows:
        cells = [r[1 + k] for k in order]
        cells.insert(foreign_at, "9")
        q += r[0] + "\t" + "\t".join(cells) + "\n"
    return db, q


@pytest.mark.parametrize("T,M", [(0, 1), (3, 1), (3, 20), (40, 1)])
def test_the_query_over_a_split_table(tmp_path, T, M):
    db, q = split_generated()
    (tmp_path / "db.tsv").write_text(db)
    (tmp_path / "new.tsv").write_text(q)
    extra = ["--min-compared", str(M)] if M != 1 else []
    prefix = str(tmp_path / "q")
    out, err = run("dists", "-t", str(tmp_path / "db.tsv"), "--query", str(tmp_path / "new.tsv"), "-o", prefix, "--within", str(T), *extra)
    al = within_ref.align(db, q)
    assert (al.D, len(al.accs), al.common, al.only_table, al.only_query) == (60, 70, 39, 1, 1)
    differ, compared = matrices(al.cells, len(al.loci))
    want = within_ref.query_tsv(al.accs, 60, differ, compared, T, M)
    got = read_files(prefix)
    assert got == {"query.tsv": want}
    near = within_ref.neighbours(differ, compared, 60, T, M)
    assert dists_lines(err) == [query_line(prefix, 10, 60, al, str(tmp_path / "db.tsv"), str(tmp_path / "new.tsv"), sum(map(len, near)), T, M,
                                           sum(1 for n in near if not n))]
    # ... and the lines with a query accession of a --within run over the aligned and concatenated table, put in the query's order
    (tmp_path / "both.tsv").write_text(within_ref.table_text(al.accs, al.loci, al.cells))
    run("dists", "-t", str(tmp_path / "both.tsv"), "-o", str(tmp_path / "b"), "--no-matrices", "--within", str(T), *extra)
    row = {name: k for k, name in enumerate(al.accs)}
    mine = {k: [] for k in range(60, 70)}
    for line in open(tmp_path / "b.within.tsv").read().splitlines()[1:]:
        a, b, d, c = line.split("\t")
        for x, y in ((row[a], row[b]), (row[b], row[a])):
            if x >= 60:
                mine[x].append((int(d), -int(c), y))
    again = "query\tneighbour\tin\tdiffer\tcompared\n"
    for k in range(60, 70):
        if not mine[k]:
            again += f"{al.accs[k]}\t-\t-\t-\t-\n"
        for dd, c, y in sorted(mine[k]):
            again += f"{al.accs[k]}\t{al.accs[y]}\t{'table' if y < 60 else 'query'}\t{dd}\t{-c}\n"
    assert again == want


def test_tables_that_need_no_gpu_write_their_headers(tmp_path):
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")
    p = subprocess.run([BIN, "dists", "-t", str(tmp_path / "noloci.tsv"), "-o", str(tmp_path / "n"), "--within", "2", "--no-matrices"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert read_files(tmp_path / "n") == {"within.tsv": "a\tb\tdiffer\tcompared\n"}
    assert dists_lines(p.stderr)[-1] == within_line(str(tmp_path / "n"), 0, 2, 1)
