"""`colorid dists --mst [--cluster T] [--min-compared M] [--no-matrices]` and `search -s -m --alleles PREFIX --dists --mst` end to end:
PREFIX.mst.tsv and PREFIX.mst.nwk against tests/mst_ref.py over matrices derived from the table's text, the other files against a run
without --mst, the forest cut at T against clusters.tsv, the closing line of stderr against the reference's numbers.  The table of
tests/golden/alleles, the generated 70 x 40 table of test_gpu_cli_dists.py with some names that need Newick quotes, the four-phage scheme
through the search's own context, an empty table and a table without loci."""
import os
import subprocess

import pytest

import mst_ref
from test_gpu_cli_alleles import BIN, run
from test_gpu_cli_alleles import env  # noqa: F401  (the module-scoped fixture: the four-phage index and its scheme)
from test_gpu_cli_dists import GOLD, generated_table, matrices, parse_table

pytestmark = pytest.mark.gpu

EXTS = ("dists.tsv", "compared.tsv", "clusters.tsv", "mst.tsv", "mst.nwk")


def read_files(prefix):
    return {ext: open(f"{prefix}.{ext}").read() for ext in EXTS if os.path.exists(f"{prefix}.{ext}")}


def reference(text, M=1):
    """(accessions, edges, {mst.tsv, mst.nwk}) of a table's text"""
    accs, loci, cells = parse_table(text)
    differ, compared = matrices(cells, len(loci))
    edges = mst_ref.forest(differ, compared, M)
    return accs, edges, {"mst.tsv": mst_ref.mst_tsv(accs, edges), "mst.nwk": mst_ref.mst_nwk(accs, edges)}


def forest_line(err, prefix, accs, edges):
    lines = [l for l in err.splitlines() if l.startswith("dists: ")]
    trees, n, length = mst_ref.summary(len(accs), edges)
    assert lines[-1] == (f"dists: minimum spanning forest: {trees} trees, {n} edges, total length {length}, "
                         f"written to {prefix}.mst.tsv, {prefix}.mst.nwk")
    return lines


def clusters_of(text):
    """clusters.tsv -> per accession its cluster number"""
    return [int(l.split("\t")[1]) for l in text.splitlines()[1:]]


def same_partition(numbers, roots):
    return len(set(zip(numbers, roots))) == len(set(numbers)) == len(set(roots))


def quoted_table():
    text, accs = generated_table()
    for old, new in (("iso_5\t", "iso'5\t"), ("iso_6\t", "iso(6)\t"), ("iso_8\t", "p:q\t"), ("iso_9\t", "it's, [9];\t")):
        assert text.count("\n" + old) == 1
        text = text.replace("\n" + old, "\n" + new)
    return text


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_mst")
    (d / "gen.tsv").write_text(quoted_table())
    return d, {"gold": (GOLD, open(GOLD).read()), "gen": (str(d / "gen.tsv"), quoted_table())}


@pytest.mark.parametrize("which,T,M", [("gold", 1, None), ("gen", 0, None), ("gen", 3, None), ("gen", 3, 20)])
def test_mst_files_and_the_files_beside_them(tables, which, T, M):
    d, t = tables
    path, text = t[which]
    extra = ["--min-compared", str(M)] if M is not None else []
    plain, with_mst, bare, only = (str(d / f"{which}{T}{M}{k}") for k in "pmbo")
    run("dists", "-t", path, "-o", plain, "--cluster", str(T), *extra)
    out, err = run("dists", "-t", path, "-o", with_mst, "--cluster", str(T), "--mst", *extra)
    accs, edges, want = reference(text, M or 1)
    got = read_files(with_mst)
    assert sorted(got) == sorted(EXTS)
    assert got["mst.tsv"] == want["mst.tsv"] and got["mst.nwk"] == want["mst.nwk"]
    before = read_files(plain)
    assert sorted(before) == ["clusters.tsv", "compared.tsv", "dists.tsv"] and all(got[k] == before[k] for k in before)
    lines = forest_line(err, with_mst, accs, edges)
    assert len(lines) == 3 and lines[0].endswith(f"written to {with_mst}.dists.tsv, {with_mst}.compared.tsv")
    # the forest cut at T spans exactly the clusters
    assert same_partition(clusters_of(got["clusters.tsv"]), mst_ref.cut(len(accs), edges, T))
    if which == "gen":
        assert "'iso 0'" in got["mst.nwk"] and "'iso''5'" in got["mst.nwk"] and "'it''s, [9];'" in got["mst.nwk"] and "iso_1" in got["mst.nwk"]
        assert not any({lo, hi} in ({0, 1}, {2, 3}) for lo, hi, _, _ in edges)     # no locus in common: never an edge
    # --no-matrices: the same bytes, without the two matrices
    out, err = run("dists", "-t", path, "-o", bare, "--cluster", str(T), "--mst", "--no-matrices", *extra)
    assert read_files(bare) == {k: got[k] for k in ("clusters.tsv", "mst.tsv", "mst.nwk")}
    lines = forest_line(err, bare, accs, edges)
    assert lines[0] == f"dists: {len(accs)} accessions x {len(parse_table(text)[1])} loci, matrices not written (--no-matrices)" and len(lines) == 3
    out, err = run("dists", "-t", path, "-o", only, "--mst", "--no-matrices", *extra)
    assert read_files(only) == {k: got[k] for k in ("mst.tsv", "mst.nwk")}
    assert len(forest_line(err, only, accs, edges)) == 2


def test_the_golden_forest_by_hand(tmp_path):
    """tests/golden/alleles by hand.  Nothing differs between acc_A and acc_B (lmo0001), acc_A and acc_late (Zlocus), acc_C and sample 4
    (lmo0001), one shared locus each; at one difference acc_A - acc_C comes first: they share two loci (abcZ, lmo0001), every other pair one"""
    run("dists", "-t", GOLD, "-o", str(tmp_path / "g"), "--mst")
    got = read_files(tmp_path / "g")
    assert sorted(got) == ["compared.tsv", "dists.tsv", "mst.nwk", "mst.tsv"]
    assert got["mst.tsv"] == ("a\tb\tdiffer\tcompared\nacc_A\tacc_B\t0\t1\nacc_A\tacc_late\t0\t1\nacc_C\tsample 4\t0\t1\n"
                              "acc_A\tacc_C\t1\t2\n")
    assert got["mst.nwk"] == "(acc_B:0,('sample 4':0)acc_C:1,acc_late:0)acc_A;\n"
    # two shared loci asked for: acc_A - acc_C is the only edge left
    run("dists", "-t", GOLD, "-o", str(tmp_path / "m"), "--mst", "--min-compared", "2", "--no-matrices")
    assert read_files(tmp_path / "m") == {"mst.tsv": "a\tb\tdiffer\tcompared\nacc_A\tacc_C\t1\t2\n",
                                          "mst.nwk": "(acc_C:1)acc_A;\nacc_B;\nacc_late;\n'sample 4';\n"}


def test_search_dists_mst_writes_what_dists_writes_from_the_raw_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    out, err = run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "ms"), "--dists", "--mst", "--cluster", "0")
    run("dists", "-t", str(d / "ms.raw.tsv"), "-o", str(d / "ms_again"), "--mst", "--cluster", "0")
    got = read_files(d / "ms")
    assert sorted(got) == sorted(EXTS) and got == read_files(d / "ms_again")
    accs, edges, want = reference(open(d / "ms.raw.tsv").read())
    assert got["mst.tsv"] == want["mst.tsv"] and got["mst.nwk"] == want["mst.nwk"]
    forest_line(err, str(d / "ms"), accs, edges)
    # Listeria_phage_B051 and Listeria_phage_B545 share locB_4: the one pair with a common call
    assert got["mst.tsv"] == "a\tb\tdiffer\tcompared\nListeria_phage_B051\tListeria_phage_B545\t0\t1\n"
    assert got["mst.nwk"] == "Listeria_phage_B021;\nListeria_phage_B056;\n(Listeria_phage_B545:0)Listeria_phage_B051;\n"


def test_search_dists_mst_with_max_missing_takes_the_clean_table(env):  # noqa: F811
    d, bxi, files, rows, _ = env
    run("search", "-b", bxi, "-q", *files, "-s", "-m", "--alleles", str(d / "mc"), "--max-missing", "2", "--dists", "--mst", "--no-matrices")
    run("dists", "-t", str(d / "mc.clean.tsv"), "-o", str(d / "mc_again"), "--mst", "--no-matrices")
    got = read_files(d / "mc")
    accs, edges, want = reference(open(d / "mc.clean.tsv").read())
    assert accs == ["Listeria_phage_B021", "Listeria_phage_B545"]
    assert got == read_files(d / "mc_again") == want


def test_an_empty_table_and_a_table_without_loci(tmp_path):
    (tmp_path / "empty.tsv").write_text("\t\n")
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")
    for name, nwk, trees in (("empty", "", 0), ("noloci", "'acc 1';\nb;\n", 2)):
        p = subprocess.run([BIN, "dists", "-t", str(tmp_path / f"{name}.tsv"), "-o", str(tmp_path / name), "--mst", "--cluster", "2"],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        got = read_files(tmp_path / name)
        assert sorted(got) == sorted(EXTS) and got["mst.tsv"] == "a\tb\tdiffer\tcompared\n" and got["mst.nwk"] == nwk
        assert p.stderr.splitlines()[-1] == (f"dists: minimum spanning forest: {trees} trees, 0 edges, total length 0, written to "
                                             f"{tmp_path / name}.mst.tsv, {tmp_path / name}.mst.nwk")
