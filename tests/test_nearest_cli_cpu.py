"""`colorid search --nearest`: what the argument check refuses, before a GPU context is made (so these run without a GPU), and the help
text that lists the flag."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))


def refused(*args, env=None):
    clean = {k: v for k, v in os.environ.items() if k != "COLORID_REDUCE"}
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", "scheme.fasta", *args], capture_output=True, text=True, timeout=60,
                       env=dict(clean, **(env or {})))
    assert p.returncode != 0, p.stderr
    assert "Loading index" not in p.stderr and p.stdout.count("\n") == 3       # the banner and nothing else
    return p.stderr


@pytest.mark.parametrize("flags", [[], ["-s", "-m"], ["-g", "-m"], ["-s", "-m", "-p", "0.9"]], ids=lambda f: "".join(f) or "alone")
def test_nearest_needs_the_allele_table(flags):
    assert "--nearest needs -s -m --alleles PREFIX" in refused("--nearest", *flags)


@pytest.mark.parametrize("flags", [["-s"], ["-m"], ["-g", "-m"]], ids=lambda f: "".join(f))
def test_alleles_still_asks_for_the_perfect_search_per_record(flags):
    assert "--alleles" in refused("--alleles", "t", "--nearest", *flags)


@pytest.mark.parametrize("group", [["--gpus", "2"], ["--devices", "0,1"], ["--gpus", "2", "--placement", "striped"], ["--placement", "replicated"]],
                         ids=lambda g: g[0][2:] + ("-" + g[2][2:] if len(g) > 2 else ""))
def test_nearest_runs_on_one_gpu(group):
    assert "--nearest runs on one GPU" in refused("-s", "-m", "--alleles", "t", "--nearest", *group)


@pytest.mark.parametrize("value", ["host", "rccl"])
def test_nearest_does_not_go_with_the_group_route_on_one_rank(value):
    err = refused("-s", "-m", "--alleles", "t", "--nearest", env={"COLORID_REDUCE": value})
    assert "--nearest runs on one GPU" in err and "COLORID_REDUCE" in err


def test_help_lists_the_flag():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--alleles PREFIX --nearest" in p.stdout and "PREFIX.nearest.tsv" in p.stdout
