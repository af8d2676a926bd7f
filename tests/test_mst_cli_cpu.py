"""`dists --mst` and `--no-matrices` without a GPU: what does not go together is refused before "Loading index", before the table is read
and before a GPU context is made, with no output file; --min-compared goes with --mst alone; the help lists both flags; both libraries
export cid_dists_best and cid_dists_forest, and the header, the ctypes table and the Rust bindings carry them."""
import os
import subprocess

import pytest

from test_dists_cli_cpu import BANNER, BIN, FULL, ROOT, dists, no_output, refused

ALLELES = ["-s", "-m", "--alleles", "out"]


@pytest.mark.parametrize("flags", [["--mst"], ALLELES + ["--mst"], ALLELES + ["--mst", "--min-compared", "2"]], ids=lambda f: "".join(f))
def test_mst_needs_dists(flags):
    assert "--mst needs --dists" in refused(*flags)


@pytest.mark.parametrize("flags", [["--no-matrices"], ALLELES + ["--no-matrices"]], ids=lambda f: "".join(f))
def test_no_matrices_needs_dists(flags):
    assert "--no-matrices needs --dists" in refused(*flags)


def test_cluster_is_still_asked_for_dists_first():
    assert "--cluster needs --dists" in refused(*ALLELES, "--cluster", "3", "--mst")


def test_no_matrices_alone_is_refused_in_search():
    assert "--no-matrices needs --mst or --cluster" in refused(*FULL, "--no-matrices")


def test_min_compared_keeps_its_words_without_cluster_and_mst():
    assert "--min-compared needs --cluster" in refused(*FULL, "--min-compared", "5")


def test_no_matrices_alone_is_refused_before_the_table_is_read(tmp_path):
    p = dists(tmp_path, "-t", "no_such_table.tsv", "-o", "p", "--no-matrices")
    assert p.returncode != 0 and "--no-matrices needs --mst or --cluster" in p.stderr and "could not open" not in p.stderr
    (tmp_path / "t.tsv").write_text("\tl1\tl2\nA\t1\t2\nB\t1\tNA\n")
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p", "--no-matrices")
    assert p.returncode != 0 and "--no-matrices needs --mst or --cluster" in p.stderr
    p = dists(tmp_path, "-t", "t.tsv", "-o", "p", "--min-compared", "2")
    assert p.returncode != 0 and "--min-compared needs --cluster" in p.stderr
    no_output(tmp_path, ["t.tsv"])


@pytest.mark.parametrize("flags", [["--mst", "--min-compared", "2"], ["--mst", "--no-matrices"], ["--cluster", "1", "--no-matrices"],
                                   ["--mst", "--cluster", "1", "--min-compared", "1", "--no-matrices"]], ids=lambda f: "".join(f))
def test_the_flags_are_accepted_as_far_as_the_gpu(tmp_path, flags):
    """on a host without a GPU the run ends at the context, after the flags and the table; with one it writes its files"""
    (tmp_path / "t.tsv").write_text("\tl1\tl2\nA\t1\t2\nB\t1\tNA\n")
    p = subprocess.run([BIN, "dists", "-t", "t.tsv", "-o", "p", *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert " needs " not in p.stderr and p.stdout == BANNER
    if p.returncode != 0:
        assert "cannot open GPU" in p.stderr
        no_output(tmp_path, ["t.tsv"])
    else:
        made = set(os.listdir(tmp_path)) - {"t.tsv"}
        assert ("p.mst.tsv" in made) == ("--mst" in flags) and ("p.dists.tsv" in made) == ("--no-matrices" not in flags)


def test_tables_that_need_no_gpu(tmp_path):
    """no accession, or no locus: the branch that opens no cid_dists writes the forest of single accessions"""
    (tmp_path / "e.tsv").write_text("\t\n")
    p = dists(tmp_path, "-t", "e.tsv", "-o", "e", "--mst", "--no-matrices")
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "e.mst.tsv").read() == "a\tb\tdiffer\tcompared\n" and open(tmp_path / "e.mst.nwk").read() == ""
    assert [l for l in p.stderr.splitlines() if l.startswith("dists: ")] == [
        "dists: 0 accessions x 0 loci, matrices not written (--no-matrices)",
        "dists: minimum spanning forest: 0 trees, 0 edges, total length 0, written to e.mst.tsv, e.mst.nwk"]
    (tmp_path / "n.tsv").write_text("\t\nacc 1\nb\nit's\n")
    p = dists(tmp_path, "-t", "n.tsv", "-o", "n", "--mst", "--cluster", "0")
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "n.mst.tsv").read() == "a\tb\tdiffer\tcompared\n"
    assert open(tmp_path / "n.mst.nwk").read() == "'acc 1';\nb;\n'it''s';\n"
    assert open(tmp_path / "n.dists.tsv").read() == "\tacc 1\tb\tit's\nacc 1\t0\t0\t0\nb\t0\t0\t0\nit's\t0\t0\t0\n"
    lines = [l for l in p.stderr.splitlines() if l.startswith("dists: ")]
    assert lines[0] == "dists: 3 accessions x 0 loci written to n.dists.tsv, n.compared.tsv" and len(lines) == 3
    assert lines[2] == "dists: minimum spanning forest: 3 trees, 0 edges, total length 0, written to n.mst.tsv, n.mst.nwk"
    assert sorted(os.listdir(tmp_path)) == ["e.mst.nwk", "e.mst.tsv", "e.tsv", "n.clusters.tsv", "n.compared.tsv", "n.dists.tsv", "n.mst.nwk",
                                            "n.mst.tsv", "n.tsv"]


def test_help_lists_the_new_flags():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert "--mst" in p.stdout and "--no-matrices" in p.stdout and "PREFIX.mst.tsv" in p.stdout and "PREFIX.mst.nwk" in p.stdout
    assert "dists -t TABLE -o PREFIX [--cluster T] [--mst] [--min-compared M] [--no-matrices]" in p.stdout


@pytest.mark.parametrize("lib", ["libcolorid_hip.so", "libcolorid_hip_tune.so"])
def test_both_libraries_export_the_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colorid_amd", lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"cid_dists_best", "cid_dists_forest"} <= names


def test_header_ctypes_table_and_rust_bindings_carry_them():
    from colorid_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    for name in ("cid_dists_best", "cid_dists_forest"):
        assert name in SIGNATURES and f"int {name}(" in header and f"pub fn {name}(" in rust
    assert "typedef struct cid_dists_edge" in header
    assert "pub struct cid_dists_edge { pub a: u32, pub b: u32, pub differ: u32, pub compared: u32 }" in rust
