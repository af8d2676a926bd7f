"""read_id --taxon / --exclude: what the command line refuses before it makes a GPU context (these run on a machine without a GPU: a
refusal that came after cid_ctx_create would fail here with "cannot open GPU"), and the new entry points in the header, the export
map and the Rust bindings."""
import gzip
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
FASTQ = b"@r1 first\nACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
NEW = ["cid_bgzf_deflate_bound", "cid_bgzf_deflate", "cid_bgzf_deflate_dev", "cid_fastq_keep_steps", "cid_fastq_filter"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("refused")
    plain, gz = d / "reads.fastq", d / "reads.fastq.gz"
    plain.write_bytes(FASTQ)
    gz.write_bytes(gzip.compress(FASTQ))                                          # one gzip stream: no "BC" field
    return str(d), str(plain), str(gz)


def refused(*args):
    p = subprocess.run([BIN, "read_id", "-b", "no_such_index.bxi", "-n", "out", *args], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert p.returncode != 0
    assert "cannot open GPU" not in p.stderr and "no_such_index" not in p.stderr, p.stderr
    return p.stderr


def test_exclude_needs_taxon(inputs):
    d, plain, gz = inputs
    assert "--exclude needs --taxon" in refused("-q", gz, "--exclude")


def test_taxon_refuses_plain_fastq(inputs):
    d, plain, gz = inputs
    err = refused("-q", plain, "--taxon", "Listeria")
    assert "--taxon" in err and "bgzip" in err and "not compressed" in err
    assert len([ln for ln in err.splitlines() if "--taxon" in ln]) == 1           # one line that says why


def test_taxon_refuses_a_single_gzip_stream(inputs):
    d, plain, gz = inputs
    err = refused("-q", gz, "--taxon", "Listeria", "--exclude")
    assert "--taxon" in err and "bgzip" in err and "single gzip stream" in err


def test_taxon_refuses_several_gpus(inputs):
    d, plain, gz = inputs
    err = refused("-q", gz, "--taxon", "Listeria", "--gpus", "2")
    assert "--taxon" in err and "bgzip" in err and "one GPU" in err
    assert not [f for f in os.listdir(d) if f.endswith(".fq.gz")]


def test_header_export_map_and_rust_bindings_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    export = open(os.path.join(ROOT, "colorid_amd", "csrc", "export.map")).read()
    assert "global: cid_*;" in export
    for name in NEW:
        decl = re.search(r"^(CID_CORE )?(int|size_t) %s\(" % name, header, re.M)
        assert decl and not decl.group(1), f"{name}: declared in the header, as an extended entry point"
        assert re.search(r"pub fn %s\(" % name, rust), f"{name}: in include/colorid_hip.rs (tools/gen_rust_bindings.py)"
    from colorid_amd._lib import SIGNATURES
    assert all(name in SIGNATURES for name in NEW)
    assert "int cid_abi_version(void);   /* 4" in header                         # additions leave the ABI version where it is


def test_the_packages_error_codes_are_the_headers():
    from colorid_amd import _lib
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (CID_OK|CID_ERR_\w+) \(?(-?\d+)\)?", header, re.M)}
    assert len(codes) == 6
    for name, value in codes.items():
        assert getattr(_lib, name) == value, name
