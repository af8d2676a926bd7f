"""`colorid collapse` refusals: everything the collapse cannot take is refused on the host, from the command line, the input's header and
n_ref_kmers tail and the groups file, before a GPU context is made — so these run without a GPU.  The inputs are written by the oracle
(orc.Index.save).  Every refusal names the file and the accession or group, exits non-zero and writes no output file."""
import os
import subprocess

from test_subset_cpu import write_index

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))   # COLORID_BIN: e.g. a sanitizer build


def write_groups(path, pairs):
    path.write_text("".join(f"{a}\t{g}\n" for a, g in pairs))
    return str(path)


def collapse(*args):
    return subprocess.run([BIN, "collapse", *args], capture_output=True, text=True)


def refused(p, *needles):
    assert p.returncode != 0, p.stdout + p.stderr
    for n in needles:
        assert n in p.stderr, (n, p.stderr)
    # refused on the host: nothing of the collapse itself was printed and no GPU was asked for
    assert "Saving BIGSI" not in p.stdout and "Collapsing" not in p.stderr and "cannot open GPU" not in p.stderr


def no_output(tmp_path, stem="out"):
    for suffix in (".bxi", ".mxi", "_groups.tsv"):
        assert not os.path.exists(tmp_path / f"{stem}{suffix}")


def test_missing_arguments_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A2", "A")])
    refused(collapse("-i", a, "-g", g), "required arguments", "--bigsi")
    refused(collapse("-b", str(tmp_path / "out"), "-g", g), "required arguments", "--input")
    refused(collapse("-b", str(tmp_path / "out"), "-i", a), "required arguments", "--groups")
    no_output(tmp_path)


def test_more_than_one_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A")])
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, b, "-g", g), "exactly one input index", "got 2", b)
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-i", b, "-g", g), "exactly one input index", "got 2", b)
    no_output(tmp_path)


def test_missing_input_or_groups_file_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A")])
    gone = str(tmp_path / "gone.bxi")
    refused(collapse("-b", str(tmp_path / "out"), "-i", gone, "-g", g), "Can't open index!", gone)
    nofile = str(tmp_path / "nofile.tsv")
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", nofile), "can't open the groups file", nofile)
    no_output(tmp_path)


def test_truncated_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A")])
    raw = open(a, "rb").read()
    cut = str(tmp_path / "cut.bxi")
    open(cut, "wb").write(raw[:len(raw) // 2])                      # inside the row records
    refused(collapse("-b", str(tmp_path / "out"), "-i", cut, "-g", g), cut, "truncated")
    open(cut, "wb").write(raw[:-5])                                 # inside the n_ref_kmers tail
    refused(collapse("-b", str(tmp_path / "out"), "-i", cut, "-g", g), cut, "unexpected end of file")
    open(cut, "wb").write(raw[:30])                                 # inside the header
    refused(collapse("-b", str(tmp_path / "out"), "-i", cut, "-g", g), cut, "unexpected end of file")
    no_output(tmp_path)


def test_line_without_a_tab_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = tmp_path / "g.tsv"
    g.write_text("A1\tA\n\nA2 A\n")
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", str(g)), "line 3", str(g), "no TAB", "A2 A")
    no_output(tmp_path)


def test_empty_accession_or_group_name_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = tmp_path / "g.tsv"
    g.write_text("A1\tA\n\tA\n")
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", str(g)), "line 2", str(g), "empty accession name", "group A")
    g.write_text("A1\t\n")
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", str(g)), "line 1", str(g), "empty group name", "accession A1")
    g.write_text("A1\t\tignored\n")                                  # the group is what stands between the first TAB and the second
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", str(g)), "line 1", str(g), "empty group name", "accession A1")
    no_output(tmp_path)


def test_accession_listed_twice_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A2", "A"), ("A1", "B")])
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), g, "lists accession A1 twice")
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A1", "A")])   # also with the same group: a pasted line is a mistake to look at
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), g, "lists accession A1 twice")
    no_output(tmp_path)


def test_unknown_accession_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A4typo", "A")])
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), "accession A4typo", g, "is not in " + a)
    no_output(tmp_path)


def test_group_named_like_an_accession_outside_it_is_refused(orc, tmp_path):
    """two colours would carry one name: A3 stays (unlisted) or goes elsewhere, and a group of others is called A3"""
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A3"), ("A2", "A3")])                     # A3 itself is not listed: it stays as A3
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), "group A3", g, "accession A3", a, "not a member")
    g = write_groups(tmp_path / "g.tsv", [("A1", "A3"), ("A3", "elsewhere")])               # A3 is listed, into another group
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), "group A3", g, "accession A3", a, "not a member")
    no_output(tmp_path)


def test_several_gpus_and_placement_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A2", "A")])
    for flag, value in (("--gpus", "2"), ("--devices", "0,1"), ("--placement", "striped")):
        refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g, flag, value), "collapse", flag, "not provided")
    no_output(tmp_path)


def test_output_equal_to_the_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A1", "A"), ("A2", "A")])
    before = open(a, "rb").read()
    refused(collapse("-b", str(tmp_path / "a"), "-i", a, "-g", g), "the output " + str(tmp_path / "a.bxi") + " is the input " + a)
    assert open(a, "rb").read() == before
    assert not os.path.exists(tmp_path / "a_groups.tsv")


def test_accession_twice_in_the_index_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A1", "A2"])
    g = write_groups(tmp_path / "g.tsv", [("A2", "A")])
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), a, "holds accession A1 twice")
    no_output(tmp_path)


def test_minimizer_input_is_checked_alike(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.mxi", ["A1", "A2"], m_size=15)
    g = write_groups(tmp_path / "g.tsv", [("A9", "A")])
    refused(collapse("-b", str(tmp_path / "out"), "-i", a, "-g", g), "accession A9", "is not in " + a)
    no_output(tmp_path)


def test_usage_and_help_name_collapse():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode != 0 and "collapse" in p.stderr
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "collapse -b OUT -i idx.bxi -g groups.tsv" in p.stdout
