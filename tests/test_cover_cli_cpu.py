"""`colorid search --coverage`: what the argument check refuses, before a GPU context is made (so these run without a GPU), and the help
text that lists the flag."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))


def refused(*args):
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", *args], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0, p.stderr
    assert "Loading index" not in p.stderr and p.stdout.count("\n") == 3       # the banner and nothing else
    return p.stderr


@pytest.mark.parametrize("flags", [[], ["-g"], ["-m"], ["-g", "-m", "-s"], ["-s", "-m"]], ids=lambda f: "".join(f) or "alone")
def test_coverage_needs_gene_search_per_record(flags):
    assert "--coverage needs -g -m" in refused("-q", "panel.fasta", "--coverage", *flags)


@pytest.mark.parametrize("query", [["reads.fq.gz"], ["panel.fasta", "reads_R1.fastq.gz"]], ids=["gz", "fasta-and-gz"])
def test_coverage_takes_fasta_queries_only(query):
    err = refused("-q", *query, "-g", "-m", "--coverage")
    assert "--coverage takes FASTA queries, not reads" in err and query[-1] in err


@pytest.mark.parametrize("group", [["--gpus", "2"], ["--devices", "0,1"], ["--gpus", "2", "--placement", "striped"], ["--placement", "replicated"]],
                         ids=lambda g: g[0][2:] + ("-" + g[2][2:] if len(g) > 2 else ""))
def test_coverage_runs_on_one_gpu(group):
    assert "--coverage runs on one GPU" in refused("-q", "panel.fasta", "-g", "-m", "--coverage", *group)


def test_help_lists_the_flag():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "-g -m --coverage" in p.stdout
