"""search --gather: what the command line refuses before it makes a GPU context (these run on a machine without a GPU: a refusal that
came after cid_ctx_create would fail here with "cannot open GPU"), and the two new entry points in the header, the ctypes table and
the Rust bindings."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
NEW = ["cid_search_gather", "cid_search_gather_set"]


@pytest.fixture(scope="module")
def query(tmp_path_factory):
    p = tmp_path_factory.mktemp("gather_refused") / "query.fasta"
    p.write_text(">q\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    return str(p)


def refused(query, *args, **env):
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", query, *args], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", **env))
    assert p.returncode != 0
    assert "cannot open GPU" not in p.stderr and "no_such_index" not in p.stderr, p.stderr
    return p.stderr


@pytest.mark.parametrize("flags,named", [(["-g"], "-g"), (["-s"], "-s"), (["-m"], "-m"), (["-g", "-m", "--coverage"], "-g"), (["--coverage"], "--coverage"),
                                         (["--gpus", "2"], "--gpus"), (["--devices", "0,0"], "--devices"), (["--placement", "striped"], "--placement")])
def test_gather_refuses_what_it_does_not_go_with(query, tmp_path, flags, named):
    err = refused(query, "--gather", str(tmp_path / "out"), *flags)
    line = [ln for ln in err.splitlines() if "--gather" in ln]
    assert len(line) == 1 and named in line[0], err
    assert not os.path.exists(str(tmp_path / "out.gather.tsv"))


def test_gather_refuses_the_group_path_of_one_rank(query, tmp_path):
    err = refused(query, "--gather", str(tmp_path / "out"), COLORID_REDUCE="host")
    assert "--gather" in err and "COLORID_REDUCE" in err


@pytest.mark.parametrize("flag", ["--gather-min", "--gather-max"])
def test_the_bounds_need_gather(query, flag):
    err = refused(query, flag, "5")
    assert flag in err and "--gather PREFIX" in err


@pytest.mark.parametrize("flag", ["--gather-min", "--gather-max"])
@pytest.mark.parametrize("value", ["0", "-3", "many", ""])
def test_the_bounds_are_counts_of_one_or_more(query, tmp_path, flag, value):
    err = refused(query, "--gather", str(tmp_path / "out"), flag, value)
    assert flag in err and "1 or more" in err
    assert not os.path.exists(str(tmp_path / "out.gather.tsv"))


def test_the_help_names_the_flags():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    for flag in ("--gather PREFIX", "--gather-min", "--gather-max"):
        assert flag in p.stdout


def test_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    from colorid_amd import _lib
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct cid_gather_row" in header and "pub struct cid_gather_row" in rust
    from colorid_amd.hip import GATHER_DTYPE
    assert GATHER_DTYPE.itemsize == 48 and GATHER_DTYPE.fields["new_kmers"][1] == 8 and GATHER_DTYPE.fields["live_before"][1] == 40
