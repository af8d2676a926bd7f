"""`dists --closest K`, `dists --query --closest K` and `search --dists --closest K` without a GPU: --closest needs --dists; a K that is no
number from 1 to 64 is refused with the limit and a pointer at --within, before any file is opened; --query needs --within T or
--closest K and with either gets as far as its files; --closest alone justifies --no-matrices and --min-compared; tables without
accessions or loci write their closest.tsv without a GPU; the help lists the flag; the libraries, the header, the ctypes table, the Rust
bindings and the switch table carry cid_dists_closest."""
import os
import subprocess

import pytest

from test_dists_cli_cpu import BANNER, BIN, FULL, ROOT, dists, no_output, refused
from test_within_cli_cpu import NEW, TABLE, refused_dists, two_tables

HEADER = "accession\tneighbour\tdiffer\tcompared\n"


@pytest.mark.parametrize("flags", [["--closest", "3"], ["-s", "-m", "--alleles", "out", "--closest", "3"]], ids=lambda f: "".join(f))
def test_closest_needs_dists(flags):
    assert "--closest needs --dists (" in refused(*flags)


@pytest.mark.parametrize("value", ["0", "65", "x", "-1", "", "3.5", "99999999999999999999"])
def test_closest_expects_1_to_64(tmp_path, value):
    """both entrances, before the index or the table is opened: neither file exists and neither is named"""
    want = f"--closest expects a number of neighbours from 1 to 64, got '{value}'"
    err = refused(*FULL, "--closest", value)
    assert want in err and "--within T" in err
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--closest", value)
    assert want in err and "--within T" in err
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p", "--closest", value)
    assert want in err
    no_output(tmp_path, [])


def test_query_without_either_flag_says_what_it_said(tmp_path):
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p")
    assert "--query needs --within T" in err and "--query needs --within T or --closest K (" in err


@pytest.mark.parametrize("flags", [["--closest", "3"], ["--closest", "3", "--within", "1"], ["--closest", "64", "--min-compared", "2"]],
                         ids=lambda f: "".join(f))
def test_query_with_closest_gets_as_far_as_the_files(tmp_path, flags):
    p = dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p", *flags)
    assert p.returncode != 0 and " needs " not in p.stderr and "could not open no_such_table.tsv" in p.stderr
    no_output(tmp_path, [])


@pytest.mark.parametrize("flags,word", [(["--mst"], "--mst"), (["--cluster", "2"], "--cluster"), (["--no-matrices"], "--no-matrices")],
                         ids=["mst", "cluster", "no-matrices"])
def test_query_with_closest_still_writes_its_one_file_alone(tmp_path, flags, word):
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p", "--closest", "3", *flags)
    assert f"--query writes PREFIX.query.tsv alone and does not go with {word}" in err


def test_the_older_refusals_are_only_longer(tmp_path):
    for err in (refused(*FULL, "--no-matrices"), refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--no-matrices")):
        assert "--no-matrices needs --mst or --cluster T or --within T (without the two matrices nothing would be written)" in err
        assert "--closest K" in err
    err = refused(*FULL, "--min-compared", "5")
    assert "--min-compared needs --cluster T (it is the least number of loci two accessions must share to be linked), --mst or --within T" in err
    assert "--closest K" in err


@pytest.mark.parametrize("flags", [["--closest", "3", "--no-matrices"], ["--closest", "3", "--min-compared", "2"],
                                   ["--closest", "1", "--within", "0", "--cluster", "1", "--mst", "--min-compared", "1", "--no-matrices"]],
                         ids=lambda f: "".join(f))
def test_closest_alone_justifies_the_other_flags(tmp_path, flags):
    """on a host without a GPU the run ends at the context, after the flags and the table; with one it writes its files"""
    (tmp_path / "t.tsv").write_text(TABLE)
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "-o", "p", *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["t.tsv"])
    else:
        assert "p.closest.tsv" in os.listdir(tmp_path) and ("p.dists.tsv" in os.listdir(tmp_path)) == ("--no-matrices" not in flags)
        assert open(tmp_path / "p.closest.tsv").read().startswith(HEADER)
    # search: the flags pass, the index does not open
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", "scheme.fasta", *FULL, *flags], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert p.returncode != 0 and " needs " not in p.stderr and " expects " not in p.stderr


def test_a_query_with_closest_gets_as_far_as_the_gpu(tmp_path):
    two_tables(tmp_path)
    assert NEW.startswith("\tl2\tl9\n")
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "--query", "n.tsv", "-o", "p", "--closest", "1"], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["n.tsv", "t.tsv"])
    else:
        assert open(tmp_path / "p.query.tsv").read() == "query\tneighbour\tin\tdiffer\tcompared\nN1\tA\ttable\t0\t1\n"


def test_tables_that_need_no_gpu(tmp_path):
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")     # a table without loci; and one without accessions
    (tmp_path / "empty.tsv").write_text("\t\n")
    for name, A in (("noloci", 2), ("empty", 0)):
        p = dists(tmp_path, "-t", f"{name}.tsv", "-o", name, "--closest", "3", "--no-matrices")
        assert p.returncode == 0, p.stderr
        assert open(tmp_path / f"{name}.closest.tsv").read() == HEADER + ("acc 1\t-\t-\t-\nb\t-\t-\t-\n" if A else "")
        assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
            f"dists: {A} accessions x 0 loci, matrices not written (--no-matrices)",
            f"dists: {A} accessions, the 3 closest of each (at least 1 shared): {A} lines, {A} accessions without a neighbour, written to {name}.closest.tsv"]
    two_tables(tmp_path, new="\tl2\tl9\n")                     # a query table without accessions
    p = dists(tmp_path, "-t", "t.tsv", "--query", "n.tsv", "-o", "q", "--closest", "3", "--within", "2", "--min-compared", "2")
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "q.query.tsv").read() == "query\tneighbour\tin\tdiffer\tcompared\n"
    assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
        "dists: 0 query accessions against 2, 1 loci in common (1 only in t.tsv, 1 only in n.tsv); 0 neighbours, the 3 closest of each within 2 "
        "differing loci (at least 2 shared), 0 queries without one, written to q.query.tsv"]
    assert sorted(os.listdir(tmp_path)) == ["empty.closest.tsv", "empty.tsv", "n.tsv", "noloci.closest.tsv", "noloci.tsv", "q.query.tsv", "t.tsv"]


def test_help_lists_the_flag():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--dists --closest K [--within T] [--min-compared M]" in p.stdout and "PREFIX.closest.tsv" in p.stdout
    assert "dists -t TABLE --query TABLE2 -o PREFIX --closest K [--within T] [--min-compared M]" in p.stdout
    assert "dists -t TABLE --query TABLE2 -o PREFIX --within T [--min-compared M]" in p.stdout      # the older form is still there


@pytest.mark.parametrize("lib", ["libcolorid_hip.so", "libcolorid_hip_tune.so"])
def test_both_libraries_export_the_entry_point(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colorid_amd", lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "cid_dists_closest" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_ctypes_table_rust_bindings_and_switch_table_carry_it():
    from colorid_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    assert "cid_dists_closest" in SIGNATURES and "int cid_dists_closest(" in header and "pub fn cid_dists_closest(" in rust
    assert "#define CID_DISTS_CLOSEST_MAX 64u" in header and "CID_DISTS_CLOSEST_MAX" in rust
    switches = open(os.path.join(ROOT, "colorid_amd", "csrc", "cid_switches.def")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cid_dists_closest" in [l for l in switches.splitlines() if l.startswith("CID_SWITCH(dense_report_bytes")][0]
    assert "cid_dists_closest" in [l for l in readme.splitlines() if "CID_DENSE_REPORT_BYTES" in l][0]
