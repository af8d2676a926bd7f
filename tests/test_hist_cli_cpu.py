"""`dists --hist`, `dists --levels T1,T2,..` and `search --dists --hist --levels ..` without a GPU: either flag needs --dists and neither
goes with --query; a --levels list that is not 1 to 32 different numbers of loci is refused with the limit, before any file is opened;
either flag alone justifies --no-matrices and --min-compared, and the two older refusals only grew at their ends; tables without
accessions or loci write their files without a GPU; the help lists the flags; the libraries, the header, the ctypes table and the Rust
bindings carry cid_dists_hist."""
import os
import subprocess

import pytest

from test_dists_cli_cpu import BANNER, BIN, FULL, ROOT, dists, no_output, refused
from test_within_cli_cpu import TABLE, refused_dists

HIST_HEADER = "loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n"


@pytest.mark.parametrize("flags,word", [(["--hist"], "--hist"), (["-s", "-m", "--alleles", "out", "--hist"], "--hist"),
                                        (["--levels", "3"], "--levels"), (["-s", "-m", "--alleles", "out", "--levels", "0,2"], "--levels")],
                         ids=lambda f: "".join(f) if isinstance(f, list) else f)
def test_the_flags_need_dists(flags, word):
    assert f"{word} needs --dists (" in refused(*flags)


@pytest.mark.parametrize("flags,word", [(["--hist"], "--hist"), (["--levels", "3"], "--levels"), (["--closest", "2", "--hist"], "--hist"),
                                        (["--within", "1", "--levels", "0,1"], "--levels")], ids=lambda f: "".join(f) if isinstance(f, list) else f)
def test_query_stays_a_neighbour_list(tmp_path, flags, word):
    err = refused_dists(tmp_path, "-t", "no_such_table.tsv", "--query", "no_such_query.tsv", "-o", "p", *flags)
    if "--within" in flags or "--closest" in flags:
        assert f"--query writes PREFIX.query.tsv alone and does not go with {word}" in err
    else:
        assert "--query needs --within T or --closest K (" in err
    no_output(tmp_path, [])


@pytest.mark.parametrize("value", ["", "3,,4", "-1", "x", "2,2", ",".join(str(k) for k in range(33)), "3,", ",3", "1,2.5", "1, 2",
                                   "99999999999999999999"])
def test_a_bad_list_of_levels_is_refused_before_a_file_is_opened(tmp_path, value):
    want = f"--levels expects 1 to 32 different numbers of loci (0 or more) separated by commas, as in 0,2,7, got '{value}'"
    assert want in refused(*FULL, "--levels", value)
    assert want in refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--levels", value)
    no_output(tmp_path, [])


@pytest.mark.parametrize("flags", [["--no-matrices", "--hist"], ["--min-compared", "5", "--levels", "3"], ["--no-matrices", "--levels", "7,0,2"],
                                   ["--min-compared", "5", "--hist"], ["--levels", ",".join(str(k) for k in range(32)), "--hist", "--mst"]],
                         ids=lambda f: "".join(f)[:40])
def test_either_flag_justifies_the_older_ones(tmp_path, flags):
    p = dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", *flags)
    assert p.returncode != 0 and " needs " not in p.stderr and " expects " not in p.stderr and "could not open no_such_table.tsv" in p.stderr
    no_output(tmp_path, [])
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", "scheme.fasta", *FULL, *flags], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert p.returncode != 0 and " needs " not in p.stderr and " expects " not in p.stderr


def test_the_older_refusals_are_only_longer(tmp_path):
    for err in (refused(*FULL, "--no-matrices"), refused_dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--no-matrices")):
        assert ("--no-matrices needs --mst or --cluster T or --within T (without the two matrices nothing would be written), or --closest K, "
                "--hist or --levels T1,T2,..") in err
    err = refused(*FULL, "--min-compared", "5")
    assert ("--min-compared needs --cluster T (it is the least number of loci two accessions must share to be linked), --mst or --within T, "
            "or --closest K, --hist or --levels T1,T2,..") in err


def test_a_table_gets_as_far_as_the_gpu(tmp_path):
    """on a host without a GPU the run ends at the context, after the flags and the table; with one it writes its files"""
    (tmp_path / "t.tsv").write_text(TABLE)
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "-o", "p", "--hist", "--levels", "1,0", "--no-matrices"], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["t.tsv"])
    else:
        assert open(tmp_path / "p.hist.tsv").read() == HIST_HEADER + "0\t1\t1\t0\n1\t0\t1\t1\n2\t0\t1\t0\n"
        assert open(tmp_path / "p.levels.tsv").read() == "accession\tT1\tT0\taddress\nA\t1\t1\t1.1\nB\t1\t1\t1.1\n"
        no_output(tmp_path, ["p.hist.tsv", "p.levels.tsv", "t.tsv"])


def test_tables_that_need_no_gpu(tmp_path):
    (tmp_path / "noloci.tsv").write_text("\t\nacc 1\nb\n")     # a table without loci; and one without accessions
    (tmp_path / "empty.tsv").write_text("\t\n")
    (tmp_path / "noacc.tsv").write_text("\tl1\tl2\n")
    for name, A, L in (("noloci", 2, 0), ("empty", 0, 0), ("noacc", 0, 2)):
        p = dists(tmp_path, "-t", f"{name}.tsv", "-o", name, "--hist", "--levels", "0,5", "--no-matrices", "--min-compared", "2")
        assert p.returncode == 0, p.stderr
        assert open(tmp_path / f"{name}.hist.tsv").read() == HIST_HEADER + "".join(f"{n}\t0\t0\t0\n" for n in range(L + 1))
        assert open(tmp_path / f"{name}.levels.tsv").read() == "accession\tT5\tT0\taddress\n" + ("acc 1\t1\t1\t1.1\nb\t2\t2\t2.2\n" if A else "")
        assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
            f"dists: {A} accessions x {L} loci, matrices not written (--no-matrices)",
            f"dists: 0 pairs counted, 0 of them left out of the differ columns for sharing fewer than 2 loci, written to {name}.hist.tsv",
            f"dists: cluster addresses of {A} accessions (at least 2 shared): {A} at <= 5, {A} at <= 0 differing loci, written to {name}.levels.tsv"]
        assert not os.path.exists(tmp_path / f"{name}.mst.tsv")


def test_help_lists_the_flags():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--dists --hist [--min-compared M]" in p.stdout and "PREFIX.hist.tsv" in p.stdout
    assert "--dists --levels T1,T2,.. [--min-compared M]" in p.stdout and "PREFIX.levels.tsv" in p.stdout
    assert "[--within T] [--closest K] [--hist] [--levels T1,T2,..] as above" in p.stdout
    assert "--dists --closest K [--within T] [--min-compared M]" in p.stdout                    # the older ones are still there


@pytest.mark.parametrize("lib", ["libcolorid_hip.so", "libcolorid_hip_tune.so"])
def test_both_libraries_export_the_entry_point(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colorid_amd", lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "cid_dists_hist" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_ctypes_table_and_rust_bindings_carry_it():
    from colorid_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    assert "cid_dists_hist" in SIGNATURES and len(SIGNATURES["cid_dists_hist"][1]) == 7
    assert "int cid_dists_hist(" in header and "pub fn cid_dists_hist(" in rust
