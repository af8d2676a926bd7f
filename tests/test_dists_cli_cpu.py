"""`colorid dists` and `search -s -m --alleles PREFIX --dists` without a GPU: what does not go together is refused before "Loading index"
and before a GPU context is made; a table that cannot be read as PREFIX.raw.tsv is refused by line or name, with no output file and
without asking for a GPU; the help lists both forms; the library exports the three cid_dists_* entry points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
BANNER = "\n ************** initializing logger *****************\n\n"
FULL = ["-s", "-m", "--alleles", "out", "--dists"]


def refused(*args):
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", "scheme.fasta", *args], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0, p.stderr
    assert "Loading index" not in p.stderr and "cannot open GPU" not in p.stderr and p.stdout == BANNER
    return p.stderr


@pytest.mark.parametrize("flags", [["--dists"], ["--dists", "-s", "-m"], ["--dists", "--cluster", "3"]], ids=lambda f: "".join(f))
def test_dists_needs_the_allele_table(flags):
    assert "--dists needs -s -m --alleles PREFIX" in refused(*flags)


@pytest.mark.parametrize("flags", [["--cluster", "3"], ["-s", "-m", "--alleles", "out", "--cluster", "3"]], ids=lambda f: "".join(f))
def test_cluster_needs_dists(flags):
    assert "--cluster needs --dists" in refused(*flags)


def test_min_compared_needs_cluster():
    assert "--min-compared needs --cluster" in refused(*FULL, "--min-compared", "5")


@pytest.mark.parametrize("value", ["x", "-1", "", "3.5", "7 loci"])
def test_cluster_expects_a_number_of_loci(value):
    assert f"--cluster expects a number of loci (0 or more), got '{value}'" in refused(*FULL, "--cluster", value)


@pytest.mark.parametrize("value", ["many", "-2"])
def test_min_compared_expects_a_number_of_loci(value):
    assert f"--min-compared expects a number of loci (0 or more), got '{value}'" in refused(*FULL, "--cluster", "3", "--min-compared", value)


def dists(tmp_path, *args):
    p = subprocess.run([BIN, "dists", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "cannot open GPU" not in p.stderr and p.stdout == BANNER
    return p


def no_output(tmp_path, keep):
    assert sorted(os.listdir(tmp_path)) == sorted(keep)


def test_dists_needs_table_and_output(tmp_path):
    (tmp_path / "t.tsv").write_text("\tl1\nA\t1\n")
    for args, missing in ((["-o", "p"], "--table"), (["-t", "t.tsv"], "--output"), ([], "--table")):
        p = dists(tmp_path, *args)
        assert p.returncode != 0 and f"required arguments were not provided: {missing}" in p.stderr
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p", "--min-compared", "2")
    assert p.returncode != 0 and "--min-compared needs --cluster" in p.stderr
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p", "--cluster", "few")
    assert p.returncode != 0 and "--cluster expects a number of loci (0 or more), got 'few'" in p.stderr
    no_output(tmp_path, ["t.tsv"])


def test_a_ragged_table_is_refused_by_line(tmp_path):
    (tmp_path / "t.tsv").write_text("\tl1\tl2\tl3\nA\t1\t2\t3\n\nB\t1\tNA\nC\t1\t\t\n")
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p", "--cluster", "1")
    assert p.returncode != 0 and "t.tsv line 4 has 2 cells" in p.stderr and "3 loci" in p.stderr
    (tmp_path / "u.tsv").write_text("\tl1\tl2\nA\t1\t2\nB\t1\t2\t3\n")
    p = dists(tmp_path, "-t", "u.tsv", "-o", "p")
    assert p.returncode != 0 and "u.tsv line 3 has 3 cells" in p.stderr
    no_output(tmp_path, ["t.tsv", "u.tsv"])


def test_a_repeated_accession_is_refused_by_name(tmp_path):
    (tmp_path / "t.tsv").write_text("\tl1\tl2\nacc 1\t1\t2\nB\t1\tNA\nacc 1\t2\t2\n")
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p")
    assert p.returncode != 0 and "line 4 repeats the accession 'acc 1' of line 2" in p.stderr
    no_output(tmp_path, ["t.tsv"])


def test_a_table_without_header_is_refused(tmp_path):
    (tmp_path / "t.tsv").write_text("A\t1\t2\nB\t1\tNA\n")
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p")
    assert p.returncode != 0 and "has no header" in p.stderr
    (tmp_path / "e.tsv").write_text("")
    p = dists(tmp_path, "-t", "e.tsv", "-o", "p")
    assert p.returncode != 0 and "has no header" in p.stderr
    no_output(tmp_path, ["e.tsv", "t.tsv"])


def test_an_unreadable_file_is_refused(tmp_path):
    p = dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--cluster", "2")
    assert p.returncode != 0 and "could not open no_such_table.tsv" in p.stderr
    no_output(tmp_path, [])


def test_a_good_table_gets_as_far_as_the_gpu(tmp_path):
    """... and no further on a host without one: the table checks come first, the context after them"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    (tmp_path / "t.tsv").write_text("\tl1\tl2\nA\t1\t2\nB\t1\tNA\n")
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "-o", "p"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode != 0 and "cannot open GPU" in p.stderr
    no_output(tmp_path, ["t.tsv"])


def test_help_lists_both_forms():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "dists -t TABLE -o PREFIX" in p.stdout and "--alleles PREFIX --dists" in p.stdout
    assert "|collapse|dists|alleles>" in p.stdout and "|alleles>" in p.stdout


def test_the_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colorid_amd", "libcolorid_hip.so")], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"cid_dists_create", "cid_dists_rows", "cid_dists_destroy"} <= names
