"""`colorid alleles` (the table writer of `search -s -m --alleles`, no GPU): on the committed rows of tests/golden/alleles it reproduces,
byte for byte, the .raw.tsv, .detailed.tsv and .report.out that the reference's workflows/MLST/process_MLST.py wrote from the same rows
(the expected.* files beside them were made by that script, once); banner and warning lines are skipped; a label without '_' is
refused by name; what `search --alleles` does not go with is refused before a GPU context is made; the help lists both."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
GOLD = os.path.join(ROOT, "tests", "golden", "alleles")
BANNER = "\n ************** initializing logger *****************\n\n"
TABLES = ("raw.tsv", "detailed.tsv", "report.out")


def alleles(*args):
    return subprocess.run([BIN, "alleles", *args], capture_output=True, text=True, timeout=60)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def test_golden_rows_give_the_reference_scripts_tables(tmp_path):
    rows = read(os.path.join(GOLD, "rows.tsv")).decode()
    labels = [line.split("\t")[0] for line in rows.splitlines()]
    assert all(l.count("_") == 1 for l in labels) and "NA" not in {line.split("\t")[1] for line in rows.splitlines()}
    p = alleles("-r", os.path.join(GOLD, "rows.tsv"), "-o", str(tmp_path / "t"))
    assert p.returncode == 0, p.stderr
    assert p.stdout == BANNER
    assert p.stderr.splitlines()[-1].startswith("alleles: 5 accessions x 6 loci written")
    for ext in TABLES:
        assert read(tmp_path / f"t.{ext}") == read(os.path.join(GOLD, f"expected.{ext}")), ext
    detailed = read(tmp_path / "t.detailed.tsv").decode().splitlines()
    assert any("MULTI" in l for l in detailed) and any("NOT_CALLED" in l for l in detailed)
    assert [l.split("\t")[0] for l in detailed[1:]].index("acc_late") == 3        # its first row is the twelfth of fifteen
    assert not (tmp_path / "t.clean.tsv").exists() and not (tmp_path / "t.dropped.txt").exists()


def test_banner_and_warning_lines_are_skipped(tmp_path):
    rows = read(os.path.join(GOLD, "rows.tsv")).decode().splitlines(keepends=True)
    noisy = [BANNER, rows[0], "Warning! no kmers in query 'lmo0001_5'; maybe your kmer length is larger than your query length?\n"] + rows[1:7] + \
            ["\n", "three\tfields\tonly\n", "Warning! no kmers in query 'a\tb'; maybe\n"] + rows[7:]
    (tmp_path / "saved_stdout.txt").write_text("".join(noisy))
    p = alleles("-r", str(tmp_path / "saved_stdout.txt"), "-o", str(tmp_path / "t"))
    assert p.returncode == 0, p.stderr
    for ext in TABLES:
        assert read(tmp_path / f"t.{ext}") == read(os.path.join(GOLD, f"expected.{ext}")), ext


def test_max_missing_splits_the_raw_table(tmp_path):
    """NA cells per accession in the golden table: acc_A 3, acc_B 4, acc_C 3, acc_late 4, 'sample 4' 5"""
    raw = read(os.path.join(GOLD, "expected.raw.tsv")).decode().splitlines(keepends=True)
    for n, dropped in ((3, ["acc_B", "acc_late", "sample 4"]), (4, ["sample 4"]), (5, []), (0, ["acc_A", "acc_B", "acc_C", "acc_late", "sample 4"])):
        p = alleles("-r", os.path.join(GOLD, "rows.tsv"), "-o", str(tmp_path / f"m{n}"), "--max-missing", str(n))
        assert p.returncode == 0, p.stderr
        assert read(tmp_path / f"m{n}.raw.tsv").decode() == "".join(raw)
        assert read(tmp_path / f"m{n}.dropped.txt").decode().splitlines() == dropped
        assert read(tmp_path / f"m{n}.clean.tsv").decode() == "".join(l for l in raw if l.split("\t")[0] not in dropped)
    p = alleles("-r", os.path.join(GOLD, "rows.tsv"), "-o", str(tmp_path / "bad"), "--max-missing", "many")
    assert p.returncode != 0 and "--max-missing expects" in p.stderr and not (tmp_path / "bad.raw.tsv").exists()


def test_a_label_without_underscore_is_refused_by_name(tmp_path):
    rows = read(os.path.join(GOLD, "rows.tsv")).decode()
    (tmp_path / "rows.tsv").write_text(rows + "nounderscore\tacc_A\t100\t1.00\n" + "also-none\tacc_B\t100\t1.00\n")
    p = alleles("-r", str(tmp_path / "rows.tsv"), "-o", str(tmp_path / "t"), "--max-missing", "2")
    assert p.returncode != 0
    assert "'nounderscore'" in p.stderr and "no '_'" in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["rows.tsv"]          # no table is written


def test_no_rows_give_empty_tables(tmp_path):
    (tmp_path / "rows.tsv").write_text(BANNER)
    p = alleles("-r", str(tmp_path / "rows.tsv"), "-o", str(tmp_path / "t"))
    assert p.returncode == 0, p.stderr
    assert read(tmp_path / "t.raw.tsv") == b"\t\n" and read(tmp_path / "t.detailed.tsv") == b"\t\n" and read(tmp_path / "t.report.out") == b""
    p = alleles("-r", str(tmp_path / "no_such_file"), "-o", str(tmp_path / "u"))
    assert p.returncode != 0 and "could not open" in p.stderr


def refused(*args):
    p = subprocess.run([BIN, "search", "-b", "no_such_index.bxi", "-q", "scheme.fasta", *args], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0, p.stderr
    assert "Loading index" not in p.stderr and p.stdout == BANNER
    return p.stderr


@pytest.mark.parametrize("flags", [[], ["-s"], ["-m"]], ids=lambda f: "".join(f) or "alone")
def test_alleles_needs_perfect_search_per_record(flags):
    assert "--alleles needs -s -m" in refused("--alleles", "out", *flags)


@pytest.mark.parametrize("flags", [["-g"], ["-g", "-m"], ["-g", "-s", "-m"]], ids=lambda f: "".join(f))
def test_alleles_does_not_go_with_gene_search(flags):
    assert "does not go with -g" in refused("--alleles", "out", *flags)


@pytest.mark.parametrize("flags", [["-s", "-m"], ["-g", "-m"], []], ids=lambda f: "".join(f) or "alone")
def test_max_missing_needs_alleles(flags):
    assert "--max-missing needs --alleles" in refused("--max-missing", "3", *flags)


def test_help_lists_the_flag_and_the_command():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "-s -m --alleles PREFIX" in p.stdout and "alleles -r ROWS -o PREFIX" in p.stdout and "|alleles>" in p.stdout
