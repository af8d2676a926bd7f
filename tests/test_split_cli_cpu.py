"""read_id / batch_id --split: what the command line refuses before it makes a GPU context (these run on a machine without a GPU: a
refusal that came after cid_ctx_create would fail here with "cannot open GPU"), and the two new entry points in the header, the ctypes
table and the Rust bindings."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
FASTQ = b"@r1 first\nACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
NEW = ["cid_fastq_split", "cid_bgzf_deflate_segments", "cid_bgzf_deflate_segments_bound"]


def bgzf(text):
    """one block-gzip member (gzip header with the "BC" field) and the end-of-file block"""
    def member(t):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(t) + c.flush()
        return (b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(body) + 25) + body +
                struct.pack("<II", zlib.crc32(t), len(t)))
    return member(text) + member(b"")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("split_refused")
    plain, gz, bgz = d / "reads.fastq", d / "reads.fastq.gz", d / "reads_bgzf.fastq.gz"
    plain.write_bytes(FASTQ)
    gz.write_bytes(gzip.compress(FASTQ))                                          # one gzip stream: no "BC" field
    bgz.write_bytes(bgzf(FASTQ))
    return str(d), str(plain), str(gz), str(bgz)


def refused(*args, cmd="read_id", **env):
    p = subprocess.run([BIN, cmd, "-b", "no_such_index.bxi", *(["-n", "out"] if cmd == "read_id" else ["-T", "tag"]), *args], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", **env))
    assert p.returncode != 0
    assert "cannot open GPU" not in p.stderr and "no_such_index" not in p.stderr, p.stderr
    return p.stderr


def one_line(err, word="--split"):
    assert len([ln for ln in err.splitlines() if word in ln]) == 1, err          # one line that says why


def test_split_refuses_taxon_and_exclude(inputs):
    d, plain, gz, bgz = inputs
    err = refused("-q", bgz, "--split", "--taxon", "Listeria")
    assert "--split" in err and "--taxon" in err
    one_line(err)
    err = refused("-q", bgz, "--split", "--exclude")
    assert "--split" in err and "--exclude" in err
    one_line(err)
    err = refused("-q", bgz, "--split", "--taxon", "Listeria", "--exclude", "--gz-matches")
    assert "--split" in err and "--taxon" in err


def test_split_refuses_plain_fastq(inputs):
    d, plain, gz, bgz = inputs
    err = refused("-q", plain, "--split")
    assert "--split" in err and "bgzip" in err and "not compressed" in err
    one_line(err)


def test_split_refuses_a_single_gzip_stream(inputs):
    d, plain, gz, bgz = inputs
    err = refused("-q", gz, "--split", "--gz-matches")
    assert "--split" in err and "bgzip" in err and "single gzip stream" in err


@pytest.mark.parametrize("flag", [("--gpus", "2"), ("--devices", "0,1"), ("--placement", "striped")])
def test_split_refuses_several_gpus(inputs, flag):
    d, plain, gz, bgz = inputs
    err = refused("-q", bgz, "--split", *flag)
    assert "--split" in err and "one GPU" in err
    assert not [f for f in os.listdir(d) if f.endswith(".fq.gz") and f not in ("reads.fastq.gz", "reads_bgzf.fastq.gz")]


def test_split_refuses_the_host_front_end(inputs):
    d, plain, gz, bgz = inputs
    err = refused("-q", bgz, "--split", COLORID_DEVICE_FASTQ="0")
    assert "--split" in err and "COLORID_DEVICE_FASTQ=0" in err


def test_batch_id_split_refuses_the_same(inputs, tmp_path):
    d, plain, gz, bgz = inputs
    sheet = tmp_path / "samples.tsv"
    sheet.write_text(f"first\t{bgz}\nsecond\t{gz}\n")
    err = refused("-q", str(sheet), "--split", cmd="batch_id")
    assert "--split" in err and "single gzip stream" in err
    err = refused("-q", str(sheet), "--split", "--taxon", "x", cmd="batch_id")
    assert "--split" in err and "--taxon" in err


def test_gz_matches_needs_taxon_or_split(inputs):
    d, plain, gz, bgz = inputs
    err = refused("-q", bgz, "--gz-matches")
    assert "--gz-matches needs --taxon" in err and "--split" in err               # the words the earlier test reads, and the new mode


def test_header_ctypes_table_and_rust_bindings_agree_on_the_new_entry_points():
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
    assert re.search(r"^#define CID_SPLIT_DROP 0xFFFFFFFFu", header, re.M) and "pub const CID_SPLIT_DROP: u32 = 0xFFFFFFFF;" in rust
    assert "int cid_abi_version(void);   /* 4" in header                         # additions leave the ABI version where it is
    import colorid_amd
    assert hasattr(colorid_amd.FastqReader, "split") and hasattr(colorid_amd.Context, "bgzf_deflate_segments")
