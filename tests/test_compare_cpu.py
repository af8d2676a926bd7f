"""`colorid compare` without a GPU: the refusals that end on the host — arguments, thresholds, the input's header and n_ref_kmers tail —
before a GPU context is made, and the report's rules (the two Jaccard formulas, the greedy duplicate list) restated in Python against a
case small enough to compute by hand.  tests/test_gpu_compare.py imports the restated rules as its expectation.  The inputs are written by
the oracle (orc.Index.save)."""
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))   # COLORID_BIN: e.g. a sanitizer build


# ---------------------------------------------------------------------------------------------- the report's rules, restated

def jaccard_bits(a, b, s):
    u = a + b - s
    return 0.0 if u == 0 else s / u


def card(x, m, n):
    """the Bloom cardinality estimate of a filter with x of m bits set by n hashes"""
    return -(m / n) * math.log(1.0 - x / m)


def jaccard_kmers(a, b, s, m, n):
    """None stands for the text `nan`: a saturated union"""
    u = a + b - s
    if u == m:
        return None
    cu = card(u, m, n)
    return 0.0 if cu == 0 else max(0.0, card(a, m, n) + card(b, m, n) - cu) / cu


def greedy_duplicates(shared, t):
    """walking the colours in order: j is a duplicate when an earlier colour that is not itself a duplicate has jaccard_bits(i, j) >= t"""
    nc = len(shared)
    dup = []
    for j in range(nc):
        if any(i not in dup and jaccard_bits(int(shared[i][i]), int(shared[j][j]), int(shared[i][j])) >= t for i in range(j)):
            dup.append(j)
    return dup


def false_prob(m, k, n):
    """what `info` prints (read_id_mt_pe.rs:695-698)"""
    return (1.0 - math.e ** (-((k * (n + 0.5)) / (m - 1.0)))) ** k


def test_the_rules_on_a_case_computed_by_hand():
    # m = 8 rows, n = 2 hashes; columns A = rows {0,1,2,3}, B = rows {2,3,4,5}, C = rows {0,1,2,3} (a copy of A)
    bits = np.zeros((8, 3), np.int64)
    bits[[0, 1, 2, 3], 0] = 1
    bits[[2, 3, 4, 5], 1] = 1
    bits[[0, 1, 2, 3], 2] = 1
    shared = bits.T @ bits
    assert shared.tolist() == [[4, 2, 4], [2, 4, 2], [4, 2, 4]]
    # A, B: s = 2, u = 6 -> 1/3;  A, C: s = 4, u = 4 -> 1
    assert jaccard_bits(4, 4, 2) == 2 / 6 and jaccard_bits(4, 4, 4) == 1.0 and jaccard_bits(0, 0, 0) == 0.0
    # card(4) = -4 ln(1/2) = 2.772589, card(6) = -4 ln(1/4) = 5.545177: inter = 2 * 2.772589 - 5.545177 = 0 -> 0 (the filters overlap
    # no more than two random sets of that size would)
    assert abs(card(4, 8, 2) - 2.772589) < 1e-6 and abs(card(6, 8, 2) - 5.545177) < 1e-6
    assert abs(jaccard_kmers(4, 4, 2, 8, 2)) < 1e-12
    # a copy: card(a) + card(b) - card(u) = card(a) -> 1
    assert jaccard_kmers(4, 4, 4, 8, 2) == 1.0
    # a = 2 (rows 0,1), b = 3 (rows 1,2,3), s = 1, u = 4: card(2) = -4 ln(3/4) = 1.150728, card(3) = -4 ln(5/8) = 1.880015,
    # inter = 1.150728 + 1.880015 - 2.772589 = 0.258154 -> 0.093110
    assert abs(jaccard_kmers(2, 3, 1, 8, 2) - 0.093110) < 1e-6
    assert jaccard_kmers(0, 0, 0, 8, 2) == 0.0          # two empty filters
    assert jaccard_kmers(8, 3, 3, 8, 2) is None         # a saturated union
    # the greedy list: C copies A; at 1/3 B joins; a chain x ~ y ~ z with x !~ z keeps z (y is gone when z is looked at)
    assert greedy_duplicates(shared, 1.0) == [2]
    assert greedy_duplicates(shared, 0.3) == [1, 2]
    chain = [[4, 3, 1], [3, 4, 3], [1, 3, 4]]           # jaccard 0-1 = 1-2 = 3/5, 0-2 = 1/7
    assert greedy_duplicates(chain, 0.6) == [1]
    assert greedy_duplicates(chain, 0.1) == [1, 2]


# ---------------------------------------------------------------------------------------------- refusals on the host

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


def compare(*args):
    return subprocess.run([BIN, "compare", *args], capture_output=True, text=True)


def refused(p, *needles):
    assert p.returncode != 0, p.stdout + p.stderr
    for n in needles:
        assert n in p.stderr, (n, p.stderr)
    # refused on the host: nothing of the comparison itself was printed and no GPU was asked for
    assert "Accessions:" not in p.stdout and "Comparing" not in p.stderr and "cannot open GPU" not in p.stderr


def no_output(tmp_path, stem="out"):
    for suffix in ("_accessions.tsv", "_pairs.tsv", "_duplicates.txt"):
        assert not os.path.exists(str(tmp_path / stem) + suffix)


def test_missing_arguments_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    refused(compare("-o", str(tmp_path / "out")), "required", "--input")
    refused(compare("-i", a), "required", "--output")
    no_output(tmp_path)


def test_more_than_one_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    b = write_index(orc, tmp_path / "b.bxi", ["B1"])
    refused(compare("-o", str(tmp_path / "out"), "-i", a, b), "exactly one input index", "got 2", b)
    no_output(tmp_path)


def test_thresholds_outside_the_unit_interval_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    refused(compare("-i", a, "-o", str(tmp_path / "out"), "-t", "1.5"), "-t/--min_jaccard", "[0, 1]", "1.5")
    refused(compare("-i", a, "-o", str(tmp_path / "out"), "-d", "1.0001"), "-d/--duplicates", "[0, 1]", "1.0001")
    refused(compare("-i", a, "-o", str(tmp_path / "out"), "-t", "half"), "-t/--min_jaccard", "half")
    refused(compare("-i", a, "-o", str(tmp_path / "out"), "-d", "nan"), "-d/--duplicates", "nan")
    no_output(tmp_path)


def test_missing_input_is_refused(tmp_path):
    gone = str(tmp_path / "gone.bxi")
    refused(compare("-o", str(tmp_path / "out"), "-i", gone), "Can't open index!", gone)
    no_output(tmp_path)


def test_truncated_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    raw = open(a, "rb").read()
    cut = str(tmp_path / "cut.bxi")
    open(cut, "wb").write(raw[:len(raw) // 2])                      # inside the row records
    refused(compare("-o", str(tmp_path / "out"), "-i", cut), cut, "truncated")
    open(cut, "wb").write(raw[:-5])                                 # inside the n_ref_kmers tail
    refused(compare("-o", str(tmp_path / "out"), "-i", cut), cut, "unexpected end of file")
    open(cut, "wb").write(raw[:30])                                 # inside the header
    refused(compare("-o", str(tmp_path / "out"), "-i", cut), cut, "unexpected end of file")
    no_output(tmp_path)


def test_an_accession_held_twice_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A2"])
    refused(compare("-o", str(tmp_path / "out"), "-i", a), a, "holds accession A2 twice")
    m = write_index(orc, tmp_path / "a.mxi", ["A1", "A1"], m_size=15)
    refused(compare("-o", str(tmp_path / "out"), "-i", m), m, "holds accession A1 twice")
    no_output(tmp_path)


def test_usage_names_compare():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode != 0 and "compare" in p.stderr
