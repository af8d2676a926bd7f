"""`colorid merge` refusals: every input the merge cannot take is refused on the host, from the inputs' headers and n_ref_kmers
tails, before a GPU context is made — so these run without a GPU.  The inputs are written by the oracle (orc.Index.save)."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))   # COLORID_BIN: e.g. a sanitizer build


def write_index(orc, path, names, m=1000, n_hash=2, k=21, m_size=0, seed=0):
    rng = np.random.default_rng(seed)
    oix = orc.Index(m, n_hash, k, len(names))
    if m_size:
        oix.set_minimizer(m_size)
    rows = oix.rows()
    for r in rng.choice(m, size=min(20, m), replace=False):
        rows[r, :] = rng.integers(0, 2**32, size=oix.w32, dtype=np.uint64).astype(np.uint32)
    if len(names) % 32:
        rows[:, -1] &= np.uint32((1 << (len(names) % 32)) - 1)
    for c, name in enumerate(names):
        oix.set_color(c, name, 100 + c)
    oix.save(str(path))
    return str(path)


def merge(*args):
    return subprocess.run([BIN, "merge", *args], capture_output=True, text=True)


def refused(p, *needles):
    assert p.returncode != 0, p.stdout + p.stderr
    for n in needles:
        assert n in p.stderr, (n, p.stderr)
    # refused on the host: nothing of the merge itself was printed and no GPU was asked for
    assert "Saving BIGSI" not in p.stdout and "Merging" not in p.stderr and "cannot open GPU" not in p.stderr


@pytest.mark.parametrize("field,kw", [("bloom_size", {"m": 1001}), ("num_hash", {"n_hash": 3}), ("k_size", {"k": 23})])
def test_mismatched_parameter_is_refused(orc, tmp_path, field, kw):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1"], **kw)
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), f"{field} differs", a, b)
    assert not os.path.exists(tmp_path / "out.bxi")


def test_mismatched_minimizer_size_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.mxi", ["A1", "A2"], m_size=15)
    b = write_index(orc, tmp_path / "b.mxi", ["B1"], m_size=13)
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), "m_size differs: 15 in " + a + ", 13 in " + b)


def test_shared_accession_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A3", "shared"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1", "shared"])
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), "accession shared is in both " + a + " and " + b)
    # the same file twice is the same case
    refused(merge("-b", str(tmp_path / "out"), "-i", a, a), "accession A1 is in both")


def test_bxi_mixed_with_mxi_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1"])
    b = write_index(orc, tmp_path / "b.mxi", ["B1"], m_size=15)
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), a, b, "must all be .bxi or all .mxi")


def test_single_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1"])
    refused(merge("-b", str(tmp_path / "out"), "-i", a), "at least two input indices", "got 1")


def test_missing_arguments_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1"])
    refused(merge("-i", a, a), "required", "--bigsi")
    refused(merge("-b", str(tmp_path / "out")), "required", "--input")


def test_output_equal_to_an_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1"])
    before = open(b, "rb").read()
    refused(merge("-b", str(tmp_path / "b"), "-i", a, b), "the output " + str(tmp_path / "b.bxi") + " is the input " + b)
    # compared after resolving the path: another spelling of the same file, and a link to it
    other = os.path.join(str(tmp_path), "sub", "..", "b")
    os.makedirs(tmp_path / "sub")
    refused(merge("-b", other, "-i", a, b), "is the input " + b)
    os.symlink(b, tmp_path / "link.bxi")
    refused(merge("-b", str(tmp_path / "link"), "-i", a, b), "is the input " + b)
    assert open(b, "rb").read() == before


def test_truncated_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1", "B2", "B3"])
    raw = open(b, "rb").read()
    cut = str(tmp_path / "cut.bxi")
    open(cut, "wb").write(raw[:len(raw) // 2])                      # inside the row records
    refused(merge("-b", str(tmp_path / "out"), "-i", a, cut), cut, "truncated")
    open(cut, "wb").write(raw[:-5])                                 # inside the n_ref_kmers tail
    refused(merge("-b", str(tmp_path / "out"), "-i", a, cut), cut, "unexpected end of file")
    open(cut, "wb").write(raw[:30])                                 # inside the header
    refused(merge("-b", str(tmp_path / "out"), "-i", a, cut), cut, "unexpected end of file")


def test_too_many_colours_are_refused(orc, tmp_path):
    """the sum of the inputs' colours must stay within the library's 2^20"""
    a = write_index(orc, tmp_path / "a.bxi", [f"a{i:07d}" for i in range(600_000)], m=4)
    b = write_index(orc, tmp_path / "b.bxi", [f"b{i:07d}" for i in range(600_000)], m=4)
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), "1200000 accessions in all")


def test_usage_names_merge():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode != 0 and "merge" in p.stderr


def test_colours_out_of_name_order_are_refused(orc, tmp_path):
    """build numbers accessions in name order (build.rs:105); a file that does not cannot go through an increasing colour map"""
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B2", "B1"])
    refused(merge("-b", str(tmp_path / "out"), "-i", a, b), b, "out of name order (B2 before B1)")
