"""`colorid fold` without a GPU: every refusal happens on the host, from the input's header and n_ref_kmers tail, before a GPU context is
made; the size `-p` chooses is printed before the context is asked for, so it is checked here against a Python restatement (the divisors
of m, orc.false_prob, the smallest that passes); the identity the feature rests on — (h % m) % m' == h % m' when m' divides m — is pinned
to the oracle alone; and the integer helpers (cid_host_math.hpp) are compiled with g++.  The inputs are written by the oracle
(orc.Index.save)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_subset_cpu import BIN, write_index
from util import random_kmers

HERE = os.path.dirname(os.path.abspath(__file__))


def fold(*args):
    return subprocess.run([BIN, "fold", *args], capture_output=True, text=True)


def refused(p, *needles):
    assert p.returncode != 0, p.stdout + p.stderr
    for n in needles:
        assert n in p.stderr, (n, p.stderr)
    # refused on the host: nothing of the fold itself was printed and no GPU was asked for
    assert "Saving BIGSI" not in p.stdout and "Filter size" not in p.stdout and "Folding" not in p.stderr and "cannot open GPU" not in p.stderr


def no_output(tmp_path, stem="out"):
    assert not os.path.exists(tmp_path / f"{stem}.bxi") and not os.path.exists(tmp_path / f"{stem}.mxi")


def divisors(m):
    return [d for d in range(1, m + 1) if m % d == 0]


# ---------------------------------------------------------------------------------------------- refusals

def test_none_or_several_of_s_f_p_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    out = str(tmp_path / "out")
    refused(fold("-b", out, "-i", a), "exactly one of -s/--bloom", "-f/--factor", "-p/--max_false_positive", "got none")
    refused(fold("-b", out, "-i", a, "-s", "500", "-f", "2"), "exactly one of", "got -s, -f")
    refused(fold("-b", out, "-i", a, "-f", "2", "-p", "0.5"), "exactly one of", "got -f, -p")
    refused(fold("-b", out, "-i", a, "-s", "500", "-f", "2", "-p", "0.5"), "exactly one of", "got -s, -f, -p")
    no_output(tmp_path)


def test_missing_arguments_are_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    refused(fold("-i", a, "-f", "2"), "required", "--bigsi")
    refused(fold("-b", str(tmp_path / "out"), "-f", "2"), "required", "--input")
    b = write_index(orc, tmp_path / "b.bxi", ["B1"])
    refused(fold("-b", str(tmp_path / "out"), "-i", a, b, "-f", "2"), "exactly one input index", "got 2", b)
    no_output(tmp_path)


def test_bad_new_size_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"], m=1000)
    out = str(tmp_path / "out")
    refused(fold("-b", out, "-i", a, "-s", "0"), "-s 0", "between 1 and the 1000 of " + a)
    refused(fold("-b", out, "-i", a, "-s", "1001"), "-s 1001", "between 1 and the 1000 of " + a)
    refused(fold("-b", out, "-i", a, "-s", "2000"), "-s 2000", "between 1 and the 1000")
    # not a divisor: the nearest ones below and above are named
    refused(fold("-b", out, "-i", a, "-s", "300"), "-s 300 does not divide the Bloom size 1000 of " + a, "250 and 500")
    refused(fold("-b", out, "-i", a, "-s", "999"), "-s 999 does not divide", "500 and 1000")
    refused(fold("-b", out, "-i", a, "-s", "3"), "-s 3 does not divide", "2 and 4")
    for text in ("abc", "12x", "-5", "1e3", ""):
        refused(fold("-b", out, "-i", a, "-s", text), "expected a whole number")
    no_output(tmp_path)


def test_bad_factor_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"], m=1000)
    out = str(tmp_path / "out")
    refused(fold("-b", out, "-i", a, "-f", "0"), "-f 0", "divisor of the Bloom size 1000 of " + a)
    refused(fold("-b", out, "-i", a, "-f", "3"), "-f 3", "divisor of the Bloom size 1000 of " + a)
    refused(fold("-b", out, "-i", a, "-f", "2000"), "-f 2000", "divisor of the Bloom size 1000")
    refused(fold("-b", out, "-i", a, "-f", "two"), "expected a whole number")
    no_output(tmp_path)


def test_bound_outside_0_1_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    for text in ("0", "1", "1.5", "-0.1", "nan", "x", "0.1x"):
        refused(fold("-b", str(tmp_path / "out"), "-i", a, "-p", text), "-p " + text, "above 0 and below 1")
    no_output(tmp_path)


def test_output_equal_to_the_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2"])
    before = open(a, "rb").read()
    refused(fold("-b", str(tmp_path / "a"), "-i", a, "-f", "1"), "the output " + str(tmp_path / "a.bxi") + " is the input " + a)
    os.symlink(a, tmp_path / "link.bxi")
    refused(fold("-b", str(tmp_path / "link"), "-i", a, "-f", "2"), "is the input " + a)
    assert open(a, "rb").read() == before


def test_missing_or_truncated_input_is_refused(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.bxi", ["A1", "A2", "A3"])
    out = str(tmp_path / "out")
    gone = str(tmp_path / "gone.bxi")
    refused(fold("-b", out, "-i", gone, "-f", "2"), "Can't open index!", gone)
    raw = open(a, "rb").read()
    cut = str(tmp_path / "cut.bxi")
    open(cut, "wb").write(raw[:len(raw) // 2])                      # inside the row records
    refused(fold("-b", out, "-i", cut, "-f", "2"), cut, "truncated")
    open(cut, "wb").write(raw[:-5])                                 # inside the n_ref_kmers tail
    refused(fold("-b", out, "-i", cut, "-f", "2"), cut, "unexpected end of file")
    open(cut, "wb").write(raw[:30])                                 # inside the header
    refused(fold("-b", out, "-i", cut, "-f", "2"), cut, "unexpected end of file")
    no_output(tmp_path)


def test_minimizer_input_is_checked_alike(orc, tmp_path):
    a = write_index(orc, tmp_path / "a.mxi", ["A1", "A2"], m_size=15)
    refused(fold("-b", str(tmp_path / "out"), "-i", a, "-s", "300"), "-s 300 does not divide the Bloom size 1000 of " + a)
    no_output(tmp_path)


def test_usage_names_fold():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode != 0 and "fold" in p.stderr
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "|fold|" in p.stdout


# ---------------------------------------------------------------------------------------------- the size -p chooses

def write_sized(orc, path, m, n_hash, n_ref):
    oix = orc.Index(m, n_hash, 21, len(n_ref))
    oix.rows()[0, 0] = 1
    for c, n in enumerate(n_ref):
        oix.set_color(c, f"acc_{c:03d}", int(n))
    oix.save(str(path))
    return str(path)


def choose(orc, m, n_hash, n_ref, bound):
    """the smallest divisor of m at which every accession's predicted rate is at or under the bound, with the worst accession and its
    rate there; None when m itself misses the bound (m' = 1 predicts 1.0: (n + 0.5) / 0 rows)"""
    def rate(size, n):
        return orc.false_prob(size, n_hash, n) if size > 1 else 1.0
    for d in divisors(m):
        rates = [rate(d, n) for n in n_ref]
        if max(rates) <= bound:
            return d, int(np.argmax(rates)), max(rates)
    return None


P_CASES = [
    # (m, n_hash, n_ref_kmers, bound)
    (720720, 4, [1000, 5000, 20], 0.01),          # highly composite: 240 divisors
    (720720, 4, [1000, 5000, 20], 0.5),
    (720720, 2, [10, 11, 12, 13], 1e-6),
    (750000, 4, [40000, 38000, 42000, 41000], 0.05),
    (1 << 20, 3, [3000] * 40, 0.001),             # a power of two
    (1 << 20, 3, [0, 0, 1], 0.9),                 # next to nothing inserted: folds down to a handful of rows
    (1000003, 4, [100, 200], 0.01),               # prime: factor 1 or a single row, and a single row predicts 1.0
    (999983 * 2, 1, [300000], 0.3),               # twice a prime
    (5040, 1, [5000, 1], 0.7),
]


@pytest.mark.parametrize("m,n_hash,n_ref,bound", P_CASES)
def test_the_size_p_chooses(orc, tmp_path, m, n_hash, n_ref, bound):
    a = write_sized(orc, tmp_path / "a.bxi", m, n_hash, n_ref)
    want = choose(orc, m, n_hash, n_ref, bound)
    assert want is not None
    size, worst, rate = want
    p = fold("-b", str(tmp_path / "out"), "-i", a, "-p", repr(bound))
    # the choice is printed before the GPU context is made: it is there whether or not this machine has a GPU
    assert f"Filter size: {size} of {m} (factor {m // size})" in p.stdout, (p.stdout, p.stderr)
    line = re.search(r"^False positive bound (\S+): accession (\S+) predicts (\S+) at filter size (\d+), the highest of (\d+)$", p.stdout, re.M)
    assert line, p.stdout
    assert line.group(1) == repr(bound) and line.group(2) == f"acc_{worst:03d}" and int(line.group(4)) == size and int(line.group(5)) == len(n_ref)
    assert float(line.group(3)) == pytest.approx(rate, rel=1e-5)
    assert float(line.group(3)) <= bound
    if m == 1000003:
        assert size == m                          # a prime size cannot be folded: only factor 1 is left


@pytest.mark.parametrize("m,n_hash,n_ref,bound", [(720720, 4, [1000, 500000, 20], 0.01), (1000003, 2, [10, 2000000], 0.5),
                                                  (1000, 1, [5, 100000, 7], 0.999)])
def test_a_bound_the_input_misses_is_refused(orc, tmp_path, m, n_hash, n_ref, bound):
    a = write_sized(orc, tmp_path / "a.bxi", m, n_hash, n_ref)
    assert choose(orc, m, n_hash, n_ref, bound) is None
    worst = int(np.argmax(n_ref))
    p = fold("-b", str(tmp_path / "out"), "-i", a, "-p", repr(bound))
    refused(p, "-p " + repr(bound), a, f"its own size {m}", f"accession acc_{worst:03d}", f"({n_ref[worst]} k-mers)")
    said = float(re.search(r"predicts (\S+);", p.stderr).group(1))
    assert said == pytest.approx(orc.false_prob(m, n_hash, n_ref[worst]), rel=1e-5) and said > bound
    no_output(tmp_path)


# ---------------------------------------------------------------------------------------------- the identity, on the oracle alone

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("m,f", [(1000, 2), (1000, 5), (1000, 1000), (1000, 1), (750000, 16), (750000, 3), (7 * 11 * 13, 11), (1 << 12, 64),
                                 (3 * (1 << 10), 3)])
def test_folding_rows_is_building_at_the_smaller_size(orc, m, f, variant):
    """orc.Index(m) filled by insert, its rows OR-ed over r % (m / f), equals orc.Index(m / f) filled by the same inserts"""
    rng = np.random.default_rng(m * 31 + f + variant)
    nc, k, n_hash = 70, 21, 3
    kmers = random_kmers(rng, 400, k)
    colours = rng.integers(0, nc, size=len(kmers))
    with orc.hash_variant(variant):
        big, small = orc.Index(m, n_hash, k, nc), orc.Index(m // f, n_hash, k, nc)
        for km, c in zip(kmers, colours):
            big.insert(int(c), km.tobytes())
            small.insert(int(c), km.tobytes())
    folded = np.bitwise_or.reduce(big.rows().reshape(f, m // f, big.w32), axis=0)
    assert folded.any()
    assert np.array_equal(folded, small.rows())


# ---------------------------------------------------------------------------------------------- the integer helpers (g++)

@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "fold_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpu_shim", "fold_shim.cpp")])
    L = C.CDLL(so)
    L.shim_fold_factor.restype = C.c_uint64
    L.shim_fold_factor.argtypes = [C.c_uint64, C.c_uint64]
    L.shim_divisors_of.restype = C.c_uint64
    L.shim_divisors_of.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]
    L.shim_nearest_divisors.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def shim_divisors(shim, m):
    out = (C.c_uint64 * 4096)()
    n = shim.shim_divisors_of(m, out, 4096)
    assert n <= 4096
    return list(out[:n])


def test_fold_factor(shim):
    for m, m2, want in [(1000, 500, 2), (1000, 1000, 1), (1000, 1, 1000), (1000, 300, 0), (1000, 0, 0), (1000, 2000, 0), (0, 5, 0),
                        (2**32, 2**31, 2), (2**32, 3, 0), (2**32, 2**32, 1), (50_000_000, 5_000_000, 10)]:
        assert shim.shim_fold_factor(m, m2) == want, (m, m2)


def test_divisors_are_all_there_and_ascending(shim):
    for m in [1, 2, 3, 4, 12, 36, 97, 1000, 5040, 46875, 65536, 65537, 720720]:
        assert shim_divisors(shim, m) == divisors(m), m
    # the count from the factorisation: 2^7 5^8; 2^32; a prime; 3 x 5 x 17 x 257 x 65537
    for m, n in [(50_000_000, 8 * 9), (2**32, 33), (2**32 - 5, 2), (2**32 - 1, 2**5)]:
        d = shim_divisors(shim, m)
        assert d == sorted(set(d)) and d[0] == 1 and d[-1] == m and all(m % x == 0 for x in d)
        assert len(d) == n, (m, len(d))
        assert [m // x for x in reversed(d)] == d                               # closed under d -> m / d: none is missing on either side of sqrt(m)


def test_nearest_divisors(shim):
    lo, hi = C.c_uint64(), C.c_uint64()
    for m, s, want in [(1000, 300, (250, 500)), (1000, 500, (500, 500)), (1000, 999, (500, 1000)), (1000, 3, (2, 4)), (1000, 0, (0, 1)),
                       (1000, 1001, (1000, 0)), (97, 50, (1, 97)), (1, 1, (1, 1)), (750000, 400000, (375000, 750000))]:
        shim.shim_nearest_divisors(m, s, C.byref(lo), C.byref(hi))
        assert (lo.value, hi.value) == want, (m, s)
