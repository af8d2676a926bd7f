"""read_id --gz-matches: refused without --taxon before a GPU context is made (this runs on a machine without a GPU), and the three
entry points behind it in the header, the Rust bindings and the ctypes table."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
NEW = ["cid_bgzf_deflate_lz", "cid_bgzf_deflate_lz_dev", "cid_fastq_filter_matches"]


def refused(sub, *args):
    p = subprocess.run([BIN, sub, "-b", "no_such_index.bxi", *args], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert p.returncode != 0
    assert "cannot open GPU" not in p.stderr and "no_such_index" not in p.stderr, p.stderr
    return p.stderr


def test_gz_matches_needs_taxon(tmp_path):
    gz = tmp_path / "reads.fastq.gz"
    gz.write_bytes(b"")
    assert "--gz-matches needs --taxon" in refused("read_id", "-n", "out", "-q", str(gz), "--gz-matches")
    sheet = tmp_path / "samples.tsv"
    sheet.write_text(f"first\t{gz}\n")
    assert "--gz-matches needs --taxon" in refused("batch_id", "-T", "run", "-q", str(sheet), "--gz-matches")


def test_header_rust_bindings_and_ctypes_table_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "colorid_hip.h")).read()
    rust = open(os.path.join(ROOT, "include", "colorid_hip.rs")).read()
    assert "global: cid_*;" in open(os.path.join(ROOT, "colorid_amd", "csrc", "export.map")).read()
    for name in NEW:
        decl = re.search(r"^(CID_CORE )?int %s\(" % name, header, re.M)
        assert decl and not decl.group(1), f"{name}: declared in the header, as an extended entry point"
        assert re.search(r"pub fn %s\(" % name, rust), f"{name}: in include/colorid_hip.rs (tools/gen_rust_bindings.py)"
    from colorid_amd._lib import SIGNATURES
    assert all(name in SIGNATURES for name in NEW)
    assert SIGNATURES["cid_bgzf_deflate_lz"] == SIGNATURES["cid_bgzf_deflate"] and SIGNATURES["cid_bgzf_deflate_lz_dev"] == SIGNATURES["cid_bgzf_deflate_dev"]
    assert "int cid_abi_version(void);   /* 4" in header                         # additions leave the ABI version where it is
