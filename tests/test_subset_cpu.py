"""`colorid subset` refusals: everything the subset cannot take is refused on the host, from the input's header and n_ref_kmers tail
and from the list file, before a GPU context is made — so these run without a GPU.  The inputs are written by the oracle
(orc.Index.save)."""
import os
import subprocess

import numpy as np

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


def write_list(path, names):
    path.write_text("".join(n + "\n" for n in names))
    return str(path)


def subset(*args):
    return subprocess.run([BIN, "subset", *args], capture_output=True, text=True)


def refused(p, *needles):
    assert p.returncode != 0, p.stdout + p.stderr
    for n in needles:
        assert n in p.stderr, (n, p.stderr)
    # refused on the host: nothing of the subset itself was printed and no GPU was asked for
    assert "Saving BIGSI" not in p.stdout and "Extracting" not in p.stderr and "cannot open GPU" not in p.stderr


def no_output(tmp_path, stem="out"):
    assert not os.path.exists(tmp_path / f"{stem}.bxi") and not os.path.exists(tmp_path / f"{stem}.mxi")


def test_neither_or_both_lists_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    refused(subset("-b", str(tmp_path / "out"), "-i", a), "exactly one of -a/--accessions", "-x/--exclude", "neither")
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-a", keep, "-x", keep), "exactly one of -a/--accessions", "both")
    no_output(tmp_path)


def test_missing_arguments_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    refused(subset("-i", a, "-a", keep), "required", "--bigsi")
    refused(subset("-b", str(tmp_path / "out"), "-a", keep), "required", "--input")
    no_output(tmp_path)


def test_more_than_one_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    refused(subset("-b", str(tmp_path / "out"), "-i", a, b, "-a", keep), "exactly one input index", "got 2", b)
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-i", b, "-a", keep), "exactly one input index", "got 2", b)
    no_output(tmp_path)


def test_missing_input_or_list_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    gone = str(tmp_path / "gone.bxi")
    refused(subset("-b", str(tmp_path / "out"), "-i", gone, "-a", keep), "Can't open index!", gone)
    nolist = str(tmp_path / "nolist.txt")
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-a", nolist), "can't open the accession list", nolist)
    no_output(tmp_path)


def test_unknown_accession_is_refused_for_keep_and_for_exclude(orc, tmp_path):
    """a typo in the list must not silently keep a contaminated genome (-x) or silently drop a wanted one (-a)"""
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    lst = write_list(tmp_path / "list.txt", ["A1", "A4typo"])
    for flag in ("-a", "-x"):
        refused(subset("-b", str(tmp_path / "out"), "-i", a, flag, lst), "accession A4typo", lst, "is not in " + a)
    no_output(tmp_path)


def test_nothing_left_to_keep_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    # the whole reference list, with its file column and a repeated line: only the text before the first TAB counts
    lst = tmp_path / "all.tsv"
    lst.write_text("A1\t/x/a1.fasta\nA2\t/x/a2.fasta\n\nA3\t/x/a3_1.fq.gz\t/x/a3_2.fq.gz\nA1\t/x/other.fasta\n")
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-x", str(lst)), "nothing left to keep", str(lst), a)
    no_output(tmp_path)


def test_empty_list_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    lst = tmp_path / "empty.txt"
    for text in ("", "\n\n\r\n"):
        lst.write_text(text)
        for flag in ("-a", "-x"):
            refused(subset("-b", str(tmp_path / "out"), "-i", a, flag, str(lst)), "accession list " + str(lst) + " is empty")
    no_output(tmp_path)


def test_output_equal_to_the_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    before = open(a, "rb").read()
    refused(subset("-b", str(tmp_path / "a"), "-i", a, "-a", keep), "the output " + str(tmp_path / "a.bxi") + " is the input " + a)
    # compared after resolving the path: another spelling of the same file, and a link to it
    os.makedirs(tmp_path / "sub")
    refused(subset("-b", os.path.join(str(tmp_path), "sub", "..", "a"), "-i", a, "-a", keep), "is the input " + a)
    os.symlink(a, tmp_path / "link.bxi")
    refused(subset("-b", str(tmp_path / "link"), "-i", a, "-a", keep), "is the input " + a)
    assert open(a, "rb").read() == before


def test_truncated_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    keep = write_list(tmp_path / "keep.txt", ["A1"])
    raw = open(a, "rb").read()
    cut = str(tmp_path / "cut.bxi")
    open(cut, "wb").write(raw[:len(raw) // 2])                      # inside the row records
    refused(subset("-b", str(tmp_path / "out"), "-i", cut, "-a", keep), cut, "truncated")
    open(cut, "wb").write(raw[:-5])                                 # inside the n_ref_kmers tail
    refused(subset("-b", str(tmp_path / "out"), "-i", cut, "-a", keep), cut, "unexpected end of file")
    open(cut, "wb").write(raw[:30])                                 # inside the header
    refused(subset("-b", str(tmp_path / "out"), "-i", cut, "-a", keep), cut, "unexpected end of file")
    no_output(tmp_path)


def test_colours_out_of_name_order_are_refused(orc, tmp_path):
    """the kept colours keep their order, and the build-identity contract needs that order to be name order (build.rs:105)"""
    a = write_index(orc, tmp_path / "a.bxi", ["B2", "B1", "B3"])
    keep = write_list(tmp_path / "keep.txt", ["B1"])
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-a", keep), a, "out of name order (B2 before B1)")
    no_output(tmp_path)


def test_too_many_kept_colours_are_refused(orc, tmp_path):
    """an index wider than the library's 2^20 colours can be cut up, but no piece may be wider than that"""
    names = [f"a{i:07d}" for i in range(1_100_000)]
    a = write_index(orc, tmp_path / "a.bxi", names, m=4)
    drop = write_list(tmp_path / "drop.txt", names[:10])
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-x", drop), "1099990 accessions kept", a, "2^20")
    no_output(tmp_path)


def test_minimizer_input_is_checked_alike(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.mxi", ["A1", "A2"], m_size=15)
    lst = write_list(tmp_path / "list.txt", ["A9"])
    refused(subset("-b", str(tmp_path / "out"), "-i", a, "-a", lst), "accession A9", "is not in " + a)
    no_output(tmp_path)


def test_usage_names_subset():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode != 0 and "subset" in p.stderr
