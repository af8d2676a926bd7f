"""`colorid dists --closest K [--within T] [--min-compared M] [--no-matrices]`, `search -s -m --alleles PREFIX --dists --closest K` and
`colorid dists --query TABLE2 --closest K [--within T]` end to end: PREFIX.closest.tsv against tests/closest_ref.py over matrices derived
from the tables' text, the files beside it against a run without --closest, the query file against the first K lines per query of
within_ref.query_tsv, the stderr lines.  The table of tests/golden/alleles, the generated 70 x 40 table of test_gpu_cli_dists.py — whole,
and split into 60 database and 10 query accessions as test_gpu_cli_within.py splits it."""
import os
import subprocess

import pytest

import closest_ref
import within_ref
from test_gpu_cli_alleles import BIN, run
from test_gpu_cli_alleles import env  # noqa: F401  (the module-scoped fixture: the four-phage index and its scheme)
from test_gpu_cli_dists import GOLD, generated_table, matrices, parse_table
from test_gpu_cli_within import QUERY, dists_lines, split_generated, within_line
from test_gpu_cli_within import read_files as read_older

pytestmark = pytest.mark.gpu


def read_files(prefix):
    got = read_older(prefix)
    if os.path.exists(f"{prefix}.closest.tsv"):
        got["closest.tsv"] = open(f"{prefix}.closest.tsv").read()
    return got


def closest_line(prefix, A, K, T, M, text):
    lines = text.splitlines()[1:]
    bound = "" if T is None else f" within {T} differing loci"
    return (f"dists: {A} accessions, the {K} closest of each{bound} (at least {M} shared): {len(lines)} lines, "
            f"{sum(1 for l in lines if l.endswith(chr(9) + '-'))} accessions without a neighbour, written to {prefix}.closest.tsv")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_closest")
    text, _ = generated_table()
    (d / "gen.tsv").write_text(text)
    return d, {"gold": (GOLD, open(GOLD).read()), "gen": (str(d / "gen.tsv"), text)}


@pytest.mark.parametrize("which,K,T,M", [("gold", 1, None, 1), ("gold", 3, None, 1), ("gold", 64, None, 2), ("gold", 3, 0, 1),
                                         ("gen", 1, None, 1), ("gen", 3, None, 20), ("gen", 64, None, 1), ("gen", 3, 3, 1), ("gen", 64, 40, 20)])
def test_closest_file_and_the_files_beside_it(tables, which, K, T, M):
    d, t = tables
    path, text = t[which]
    extra = (["--min-compared", str(M)] if M != 1 else []) + (["--within", str(T)] if T is not None else [])
    plain, with_c, bare = (str(d / f"{which}{K}_{T}_{M}{k}") for k in "pcb")
    older = dists_lines(run("dists", "-t", path, "-o", plain, "--cluster", "3", "--mst", *extra)[1])
    out, err = run("dists", "-t", path, "-o", with_c, "--cluster", "3", "--mst", "--closest", str(K), *extra)
    accs, loci, cells = parse_table(text)
    differ, compared = matrices(cells, len(loci))
    want = closest_ref.closest_tsv(accs, differ, compared, K, T, M)
    got = read_files(with_c)
    before = read_files(plain)
    assert sorted(got) == sorted(list(before) + ["closest.tsv"]) and ("within.tsv" in before) == (T is not None)
    assert got["closest.tsv"] == want
    assert all(got[k] == before[k] for k in before)                                            # byte for byte
    # every accession is in the file, in table order, with no more than K lines
    firsts = [l.split("\t")[0] for l in want.splitlines()[1:]]
    assert [a for k, a in enumerate(firsts) if k == 0 or firsts[k - 1] != a] == accs and max(firsts.count(a) for a in accs) <= K
    # one more line on stderr, after the matrices' (and the pairs'), before the clusters' and the forest's
    lines = dists_lines(err)
    at = 1 if T is None else 2
    assert lines[at] == closest_line(with_c, len(accs), K, T, M, want)
    assert [l.replace(with_c, plain) for l in lines[:at] + lines[at + 1:]] == older
    if T is not None:
        assert lines[1] == within_line(with_c, len(within_ref.pairs(differ, compared, T, M)), T, M)
    if which == "gen" and T is None and M == 1:
        assert f"{accs[0]}\t{accs[1]}\t" not in want and f"{accs[2]}\t{accs[3]}\t" not in want   # no locus in common: never a neighbour
    # --no-matrices --closest K: that one file (and the pairs' with --within), the same bytes
    out, err = run("dists", "-t", path, "-o", bare, "--no-matrices", "--closest", str(K), *extra)
    alone = read_files(bare)
    assert alone.pop("closest.tsv") == want and alone == ({} if T is None else {"within.tsv": got["within.tsv"]})
    assert dists_lines(err)[0] == f"dists: {len(accs)} accessions x {len(loci)} loci, matrices not written (--no-matrices)"
    assert dists_lines(err)[-1] == closest_line(bare, len(accs), K, T, M, want) and len(dists_lines(err)) == at + 1


def test_a_run_without_closest_says_what_it_said(tables):
    d, t = tables
    out, err = run("dists", "-t", GOLD, "-o", str(d / "quiet"), "--cluster", "1", "--within", "1")
    assert len(dists_lines(err)) == 3 and "closest of each" not in err and "closest.tsv" not in err
    assert sorted(read_files(d / "quiet")) == ["clusters.tsv", "compared.tsv", "dists.tsv", "within.tsv"]


def test_search_dists_closest_writes_what_dists_writes_from_the_raw_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "sc"), "--dists", "--closest", "2")
    out2, err2 = run("dists", "-t", str(d / "sc.raw.tsv"), "-o", str(d / "sc_again"), "--closest", "2")
    got = read_files(d / "sc")
    assert sorted(got) == ["closest.tsv", "compared.tsv", "dists.tsv"] and got == read_files(d / "sc_again")
    # Listeria_phage_B051 and Listeria_phage_B545 share locB_4: the one pair with a common call; the other accessions have no neighbour
    lines = got["closest.tsv"].splitlines()
    assert lines[0] == "accession\tneighbour\tdiffer\tcompared" and len(lines) == 5
    assert "Listeria_phage_B051\tListeria_phage_B545\t0\t1" in lines and "Listeria_phage_B545\tListeria_phage_B051\t0\t1" in lines
    assert sum(1 for l in lines if l.endswith("\t-\t-\t-")) == 2
    assert dists_lines(err)[-1] == closest_line(str(d / "sc"), 4, 2, None, 1, got["closest.tsv"])
    assert dists_lines(err)[-1].replace(str(d / "sc"), str(d / "sc_again")) == dists_lines(err2)[-1]


def query_line(prefix, Q, D, al, table, query, n, K, T, M, none):
    bound = "" if T is None else f" within {T} differing loci"
    return (f"dists: {Q} query accessions against {D}, {al.common} loci in common ({al.only_table} only in {table}, {al.only_query} only in "
            f"{query}); {n} neighbours, the {K} closest of each{bound} (at least {M} shared), {none} queries without one, written to {prefix}.query.tsv")


@pytest.mark.parametrize("K,T,M", [(3, None, 1), (3, 3, 1), (64, None, 1), (1, None, 20), (64, 40, 20)])
def test_the_query_over_a_split_table(tmp_path, K, T, M):
    db, q = split_generated()
    (tmp_path / "db.tsv").write_text(db)
    (tmp_path / "new.tsv").write_text(q)
    extra = (["--min-compared", str(M)] if M != 1 else []) + (["--within", str(T)] if T is not None else [])
    prefix = str(tmp_path / "q")
    out, err = run("dists", "-t", str(tmp_path / "db.tsv"), "--query", str(tmp_path / "new.tsv"), "-o", prefix, "--closest", str(K), *extra)
    al = within_ref.align(db, q)
    assert (al.D, len(al.accs)) == (60, 70)
    differ, compared = matrices(al.cells, len(al.loci))
    # the first K lines per query of what within_ref.query_tsv gives (without --within: at a threshold no pair exceeds)
    whole = within_ref.query_tsv(al.accs, 60, differ, compared, len(al.loci) if T is None else T, M)
    want, seen = whole.split("\n")[0] + "\n", {}
    for line in whole.split("\n")[1:-1]:
        name = line.split("\t")[0]
        seen[name] = seen.get(name, 0) + 1
        if seen[name] <= K:
            want += line + "\n"
    assert want == closest_ref.query_tsv_cut(al.accs, 60, differ, compared, K, T, M)
    assert read_files(prefix) == {"query.tsv": want}
    lines = want.splitlines()[1:]
    none = sum(1 for l in lines if l.endswith("\t-"))
    assert dists_lines(err) == [query_line(prefix, 10, 60, al, str(tmp_path / "db.tsv"), str(tmp_path / "new.tsv"), len(lines) - none, K, T, M, none)]
    if T is not None and max(seen.values()) <= K:                                              # no list is that long: --within's own file
        run("dists", "-t", str(tmp_path / "db.tsv"), "--query", str(tmp_path / "new.tsv"), "-o", str(tmp_path / "w"), *extra)
        assert open(tmp_path / "w.query.tsv").read() == want


def test_beyond_the_threshold_and_without_a_shared_locus(tmp_path):
    """new_far differs from every accession of the golden table at its one shared locus or shares none: nothing lies within 0, and
    --closest alone names its nearest all the same; new_2 has no call at any of the table's loci and gets its line of dashes"""
    query = QUERY + "new_far\t7\t5\t99\n"
    (tmp_path / "new.tsv").write_text(query)
    al = within_ref.align(open(GOLD).read(), query)
    differ, compared = matrices(al.cells, len(al.loci))
    files = {}
    for name, flags in (("near", ["--within", "0"]), ("both", ["--closest", "3", "--within", "0"]), ("any", ["--closest", "3"])):
        run("dists", "-t", GOLD, "--query", str(tmp_path / "new.tsv"), "-o", str(tmp_path / name), *flags)
        files[name] = open(tmp_path / f"{name}.query.tsv").read()
    assert files["near"] == within_ref.query_tsv(al.accs, al.D, differ, compared, 0)
    assert files["both"] == closest_ref.query_tsv_cut(al.accs, al.D, differ, compared, 3, 0)
    assert files["any"] == closest_ref.query_tsv_cut(al.accs, al.D, differ, compared, 3, None)
    assert "new_far\t-\t-\t-\t-" in files["near"].splitlines() and "new_far\t-\t-\t-\t-" in files["both"].splitlines()
    far = [l for l in files["any"].splitlines() if l.startswith("new_far\t")]
    assert len(far) == 3 and all(int(l.split("\t")[3]) >= 1 for l in far) and far[0].split("\t")[1] != "-"
    for text in files.values():
        assert "new_2\t-\t-\t-\t-" in text.splitlines()


def test_tables_that_need_no_gpu_write_their_lines(tmp_path):
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")
    p = subprocess.run([BIN, "dists", "-t", str(tmp_path / "noloci.tsv"), "-o", str(tmp_path / "n"), "--closest", "2", "--no-matrices"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert read_files(tmp_path / "n") == {"closest.tsv": "accession\tneighbour\tdiffer\tcompared\nacc 1\t-\t-\t-\nb\t-\t-\t-\n"}
