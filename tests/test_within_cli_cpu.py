"""`dists --within`, `dists --query` and `search --dists --within` without a GPU: what does not go together, and two tables that cannot be
aligned, are refused with a message that names the file and the item, before a GPU context is made and with no output file; --within
alone justifies --no-matrices and --min-compared; a query table without accessions and a table without loci write their header-only
files without a GPU; the help lists the flags; the libraries, the header, the ctypes table and the Rust bindings carry cid_dists_within."""
import os
import subprocess

import pytest

from test_dists_cli_cpu import BANNER, BIN, FULL, ROOT, dists, no_output, refused

TABLE = "\tl1\tl2\nA\t1\t2\nB\t1\tNA\n"
NEW = "\tl2\tl9\nN1\t2\t4\n"


def refused_dists(tmp_path, *args):
    p = dists(tmp_path, *args)
    assert p.returncode != 0 and "could not open" not in p.stderr and "hip" not in p.stderr.lower()
    return p.stderr


def two_tables(tmp_path, table=TABLE, new=NEW):
    (tmp_path / "t.tsv").write_text(table)
    (tmp_path / "n.tsv").write_text(new)


def test_query_needs_within(tmp_path):
    assert "--query needs --within T" in refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p")


@pytest.mark.parametrize("flags,word", [(["--mst"], "--mst"), (["--cluster", "2"], "--cluster"), (["--no-matrices"], "--no-matrices")],
                         ids=["mst", "cluster", "no-matrices"])
def test_query_writes_its_one_file_alone(tmp_path, flags, word):
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p", "--within", "1", *flags)
    assert f"--query writes PREFIX.query.tsv alone and does not go with {word}" in err
    no_output(tmp_path, [])


def test_no_common_locus_is_refused_by_file(tmp_path):
    two_tables(tmp_path, new="\tl8\tl9\nN1\t2\t4\n")
    err = refused_dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1")
    assert "t.tsv and n.tsv have no locus in common" in err
    two_tables(tmp_path, table="\t\nA\nB\n")                  # a table without loci has none in common with anything
    assert "t.tsv and n.tsv have no locus in common" in refused_dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1")
    no_output(tmp_path, ["n.tsv", "t.tsv"])


def test_a_repeated_locus_is_refused_by_file_and_name(tmp_path):
    two_tables(tmp_path, new="\tl2\tl9\tl2\nN1\t2\t4\t2\n")
    assert "n.tsv repeats the locus 'l2'" in refused_dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1")
    two_tables(tmp_path, table="\tl1\tl1\nA\t1\t2\n")
    assert "t.tsv repeats the locus 'l1'" in refused_dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1")
    no_output(tmp_path, ["n.tsv", "t.tsv"])


def test_an_accession_in_both_files_is_refused_by_name(tmp_path):
    two_tables(tmp_path, new="\tl2\tl9\nN1\t2\t4\nB\t2\t4\n")
    err = refused_dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1")
    assert "the accession 'B' is in both t.tsv and n.tsv" in err
    no_output(tmp_path, ["n.tsv", "t.tsv"])


@pytest.mark.parametrize("value", ["x", "-1", "", "3.5"])
def test_within_expects_a_number_of_loci(tmp_path, value):
    assert f"--within expects a number of loci (0 or more), got '{value}'" in refused(*FULL, "--within", value)
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--within", value)
    assert f"--within expects a number of loci (0 or more), got '{value}'" in err


@pytest.mark.parametrize("flags", [["--within", "3"], ["-s", "-m", "--alleles", "out", "--within", "3"]], ids=lambda f: "".join(f))
def test_within_needs_dists(flags):
    assert "--within needs --dists" in refused(*flags)


def test_the_older_refusals_keep_their_words(tmp_path):
    assert "--no-matrices needs --mst or --cluster" in refused(*FULL, "--no-matrices")
    assert "--min-compared needs --cluster" in refused(*FULL, "--min-compared", "5")
    assert "--no-matrices needs --mst or --cluster" in refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--no-matrices")


@pytest.mark.parametrize("flags", [["--within", "1", "--no-matrices"], ["--within", "1", "--min-compared", "2"],
                                   ["--within", "0", "--cluster", "1", "--mst", "--min-compared", "1", "--no-matrices"]], ids=lambda f: "".join(f))
def test_within_alone_justifies_the_other_flags(tmp_path, flags):
    """on a host without a GPU the run ends at the context, after the flags and the table; with one it writes its files"""
    (tmp_path / "t.tsv").write_text(TABLE)
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "-o", "p", *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["t.tsv"])
    else:
        assert "p.within.tsv" in os.listdir(tmp_path) and ("p.dists.tsv" in os.listdir(tmp_path)) == ("--no-matrices" not in flags)


def test_a_query_gets_as_far_as_the_gpu(tmp_path):
    two_tables(tmp_path)
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--within", "1"], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["n.tsv", "t.tsv"])
    else:
        assert open(tmp_path / "p.query.tsv").read() == "query\tneighbour\tin\tdiffer\tcompared\nN1\tA\ttable\t0\t1\n"


def test_tables_that_need_no_gpu(tmp_path):
    two_tables(tmp_path, new="\tl2\tl9\n")                     # a query table without accessions
    p = dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "q", "--within", "3", "--min-compared", "2")
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "q.query.tsv").read() == "query\tneighbour\tin\tdiffer\tcompared\n"
    assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
        "dists: 0 query accessions against 2, 1 loci in common (1 only in t.tsv, 1 only in n.tsv); 0 neighbours within 3 differing loci "
        "(at least 2 shared), 0 queries without one, written to q.query.tsv"]
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")     # a table without loci; and one without accessions
    (tmp_path / "empty.tsv").write_text("\t\n")
    for name, A in (("noloci", 2), ("empty", 0)):
        p = dists(tmp_path, "-t", f"{name}.tsv", "-o", name, "--within", "0", "--no-matrices")
        assert p.returncode == 0, p.stderr
        assert open(tmp_path / f"{name}.within.tsv").read() == "a\tb\tdiffer\tcompared\n"
        assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
            f"dists: {A} accessions x 0 loci, matrices not written (--no-matrices)",
            f"dists: 0 pairs within 0 differing loci (at least 1 shared), written to {name}.within.tsv"]
    assert sorted(os.listdir(tmp_path)) == ["empty.tsv", "empty.within.tsv", "n.tsv", "noloci.tsv", "noloci.within.tsv", "q.query.tsv", "t.tsv"]


def test_help_lists_the_new_flags():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--within T" in p.stdout and "PREFIX.within.tsv" in p.stdout and "PREFIX.query.tsv" in p.stdout
    assert "dists -t TABLE --query TABLE2 -o PREFIX --within T [--min-compared M]" in p.stdout


@pytest.mark.parametrize("lib", ["libcolorid_hip.so", "libcolorid_hip_tune.so"])
def test_both_libraries_export_the_entry_point(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colorid_amd", lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "cid_dists_within" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_ctypes_table_and_rust_bindings_carry_it():
    from colorid_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    assert "cid_dists_within" in SIGNATURES and "int cid_dists_within(" in header and "pub fn cid_dists_within(" in rust
    assert "#define CID_DISTS_UPPER 1u" in header and "CID_DISTS_UPPER" in rust
