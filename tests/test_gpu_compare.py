"""`colorid compare` and cid_pairs_* on the GPU.  The contract is the counter matrix shared[i][j] = popcount(column i & column j) of the
index's bit matrix, exact.  The expectation never comes from the code under test: it is numpy on rows the oracle (or numpy) made —
bits = unpackbits(rows), shared = bits^T bits (int64; wide or tall inputs in row chunks of 2^19 as a float32 product, exact because a
chunk's counts stay below 2^24, summed in int64) — and the report's rules restated in tests/test_compare_cpu.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import colorid_amd
from colorid_amd import CidError
from test_compare_cpu import false_prob, greedy_duplicates, jaccard_bits, jaccard_kmers
from test_gpu_merge import header_bytes, random_names, records_of, shuffle_records
from util import random_index, to_hip_index

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
REFS = os.path.join(HERE, "golden", "refs")
BANNER = "\n ************** initializing logger *****************\n\n"
PHAGES = [f"Listeria_phage_{n}" for n in ("B021", "B051", "B056", "B545")]


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout[len(BANNER):], p.stderr


def read(path):
    with open(path, "rb") as f:
        return f.read()


def gram(rows, nc):
    """numpy's matrix: rows is m x w32 uint32 (BitVec<u32> storage)"""
    rows = np.ascontiguousarray(rows)
    m = rows.shape[0]
    if nc <= 1000 and m <= 100_000:
        bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :nc].astype(np.int64)
        return (bits.T @ bits).astype(np.uint64)
    out = np.zeros((nc, nc), np.int64)
    for r0 in range(0, m, 1 << 19):
        bits = np.unpackbits(rows[r0:r0 + (1 << 19)].view(np.uint8), axis=1, bitorder="little")[:, :nc].astype(np.float32)
        out += (bits.T @ bits).astype(np.int64)
    return out.astype(np.uint64)


def popcounts(rows, nc):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :nc].sum(axis=0, dtype=np.int64).astype(np.uint64)


def file_records(path):
    start, n_rows, rec = header_bytes(path)
    return read(path)[start:start + n_rows * rec], rec


def pieces(raw, rec, n):
    """the records cut into n calls of (nearly) equal record counts"""
    n_rec = len(raw) // rec
    cuts = [n_rec * i // n for i in range(n + 1)]
    return [raw[cuts[i] * rec:cuts[i + 1] * rec] for i in range(n)]


def counted(ctx, m, nc, chunks):
    pr = colorid_amd.Pairs(ctx, m, nc)
    for c in chunks:
        pr.add_records(c)
    got = pr.fetch()
    pr.close()
    return got


# ---------------------------------------------------------------------------------------------- 1. the ABI, exact

WIDTHS = (1, 31, 32, 33, 64, 65, 257, 1000, 8300)


@pytest.mark.parametrize("nc", WIDTHS)
@pytest.mark.parametrize("density", [0.02, 0.3, 0.9])
@pytest.mark.parametrize("shuffle", [False, True])
def test_add_records_counts_what_numpy_counts(orc, hip_ctx, tmp_path, nc, density, shuffle):
    rng = np.random.default_rng(nc * 13 + int(density * 100) + shuffle)
    m = 300 if nc > 8192 else 600
    oix = random_index(orc, rng, m, 3, 21, nc, density=density, zero_row_frac=0.3)
    path = str(tmp_path / "in.bxi")
    oix.save(path)
    if shuffle:
        shuffle_records(path, rng)
    raw, rec = file_records(path)
    want = gram(oix.rows(), nc)
    assert np.array_equal(np.diag(want), popcounts(oix.rows(), nc))
    for n_calls in (1, 2, 3):
        got = counted(hip_ctx, m, nc, pieces(raw, rec, n_calls))
        assert got.shape == (nc, nc) and got.dtype == np.uint64
        assert np.array_equal(got, want), (n_calls, np.argwhere(got != want)[:5])
        assert np.array_equal(got, got.T)
        assert np.array_equal(np.diag(got), popcounts(oix.rows(), nc))


def test_many_tiles_per_workgroup(orc, hip_ctx, tmp_path):
    """rows enough that a workgroup walks several row tiles (and the last one a short range), three 64-colour blocks"""
    rng = np.random.default_rng(77)
    m, nc = 300_007, 130
    oix = random_index(orc, rng, m, 3, 21, nc, density=0.4, zero_row_frac=0.2)
    path = str(tmp_path / "in.bxi")
    oix.save(path)
    raw, rec = file_records(path)
    want = gram(oix.rows(), nc)
    assert np.array_equal(counted(hip_ctx, m, nc, [raw]), want)
    hx = to_hip_index(hip_ctx, oix)
    pr = colorid_amd.Pairs(hip_ctx, m, nc)
    pr.add_index(hx)
    assert np.array_equal(pr.fetch(), want)
    pr.close()
    hx.close()


# ---------------------------------------------------------------------------------------------- 2. the two sources agree

@pytest.mark.parametrize("nc", [1, 33, 64, 65, 257, 1000])
def test_resident_index_and_records_agree_and_calls_accumulate(orc, hip_ctx, tmp_path, nc):
    rng = np.random.default_rng(nc + 5)
    m = 2000
    oix = random_index(orc, rng, m, 3, 21, nc, density=0.3, zero_row_frac=0.3)
    path = str(tmp_path / "in.bxi")
    oix.save(path)
    raw, _ = file_records(path)
    want = gram(oix.rows(), nc)
    hx = to_hip_index(hip_ctx, oix)                    # resident: all m rows, the zero ones included
    a, b = colorid_amd.Pairs(hip_ctx, m, nc), colorid_amd.Pairs(hip_ctx, m, nc)
    a.add_index(hx)
    b.add_records(raw)
    assert np.array_equal(a.fetch(), want) and np.array_equal(b.fetch(), want)
    a.add_index(hx)                                    # added, not stored: the same source again doubles every counter
    b.add_records(raw)
    assert np.array_equal(a.fetch(), 2 * want) and np.array_equal(b.fetch(), 2 * want)
    a.add_records(raw)                                 # ... and the two sources add up in one object
    assert np.array_equal(a.fetch(), 3 * want)
    a.close()
    b.close()
    hx.close()


# ---------------------------------------------------------------------------------------------- 3. chunking

@pytest.mark.parametrize("per_call", [1, 63, 64, 65, 101])
def test_any_split_of_a_file_counts_the_file(orc, hip_ctx, tmp_path, per_call):
    rng = np.random.default_rng(per_call)
    m, nc = 700, 97
    oix = random_index(orc, rng, m, 3, 21, nc, density=0.3, zero_row_frac=0.3)
    path = str(tmp_path / "in.bxi")
    oix.save(path)
    shuffle_records(path, rng)
    raw, rec = file_records(path)
    n_rec = len(raw) // rec
    whole = counted(hip_ctx, m, nc, [raw])
    assert np.array_equal(whole, gram(oix.rows(), nc))
    pr = colorid_amd.Pairs(hip_ctx, m, nc)
    for r0 in range(0, n_rec, per_call):
        pr.add_records(raw[r0 * rec:(r0 + per_call) * rec])
    assert np.array_equal(pr.fetch(), whole)
    pr.add_records(b"")                                # a call of zero records is accepted and changes nothing
    assert np.array_equal(pr.fetch(), whole)
    pr.close()


# ---------------------------------------------------------------------------------------------- 4. refusals

def test_refusals(hip_ctx):
    lib = hip_ctx.lib
    h = C.c_void_p()
    assert lib.cid_pairs_create(None, 100, 3, C.byref(h)) == -1
    assert lib.cid_pairs_create(hip_ctx.h, 100, 3, None) == -1
    assert lib.cid_pairs_create(hip_ctx.h, 0, 3, C.byref(h)) == -1 and lib.cid_pairs_create(hip_ctx.h, 100, 0, C.byref(h)) == -1
    pr = colorid_amd.Pairs(hip_ctx, 100, 3)
    out = np.zeros((3, 3), np.uint64)
    assert lib.cid_pairs_add_records(None, None, 0) == -1
    assert lib.cid_pairs_add_records(pr.h, None, 5) == -1
    assert lib.cid_pairs_add_index(pr.h, None) == -1 and lib.cid_pairs_add_index(None, None) == -1
    assert lib.cid_pairs_fetch(pr.h, None) == -1 and lib.cid_pairs_fetch(None, out.ctypes.data_as(C.c_void_p)) == -1
    lib.cid_pairs_destroy(None)
    # an index of another bloom_size / n_colors, and one that is not finalized
    for m, nc in ((101, 3), (100, 4)):
        other = colorid_amd.Index(hip_ctx, m, 2, 21, nc).finalize()
        with pytest.raises(CidError) as e:
            pr.add_index(other)
        assert e.value.code == -1
        other.close()
    raw_ix = colorid_amd.Index(hip_ctx, 100, 2, 21, 3)
    with pytest.raises(CidError) as e:
        pr.add_index(raw_ix)
    assert e.value.code == -1 and "not finalized" in str(e.value)
    # malformed records, with cid_index_put_records' text (the cases of test_put_records_subset_refusals)
    with pytest.raises(CidError) as e:                                           # two words announced, the shape has one
        pr.add_records(struct.pack("<QQIQ", 5, 2, 0b101, 3))
    assert e.value.code == -1 and "word count != ceil(n_colors/32)" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit count that is not the shape's
        pr.add_records(records_of({5: [0b101]}, 4))
    assert e.value.code == -1 and "bit count != n_colors" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a row past bloom_size
        pr.add_records(records_of({100: [0b101]}, 3))
    assert e.value.code == -1 and "row >= bloom_size" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit past the 3 colours
        pr.add_records(records_of({5: [0b1101]}, 3))
    assert e.value.code == -1 and "bits beyond n_colors" in str(e.value)
    assert not pr.fetch().any()                                                  # a refused call added nothing
    pr.add_records(records_of({5: [0b101], 99: [0b110]}, 3))
    assert pr.fetch().tolist() == [[1, 0, 1], [0, 1, 1], [1, 1, 2]]
    raw_ix.put_rows([5, 99], [[0b101], [0b110]])
    raw_ix.finalize()
    pr.add_index(raw_ix)
    assert pr.fetch().tolist() == [[2, 0, 2], [0, 2, 2], [2, 2, 4]]
    raw_ix.close()
    pr.close()


def test_counters_that_do_not_fit_are_refused_and_the_context_lives_on(hip_ctx):
    with pytest.raises(CidError) as e:
        colorid_amd.Pairs(hip_ctx, 1000, 1 << 20)                                # 8 TiB of counters
    assert e.value.code == -4 and str(8 * (1 << 40)) in str(e.value), str(e.value)
    pr = colorid_amd.Pairs(hip_ctx, 10, 2)
    pr.add_records(records_of({3: [0b11], 4: [0b10]}, 2))
    assert pr.fetch().tolist() == [[1, 1], [1, 2]]
    pr.close()


# ---------------------------------------------------------------------------------------------- the reports

def expected_reports(shared, names, n_ref, m, n_hash, t=0.0):
    """(accession rows, pair rows) as the CLI writes them: strings and integers as they are, the %.6f fields as floats (None: `nan`)"""
    nc = len(names)
    bits = [int(shared[c][c]) for c in range(nc)]
    acc = [(names[c], int(n_ref[c]), bits[c], bits[c] / m, false_prob(float(m), float(n_hash), float(n_ref[c])), (bits[c] / m) ** n_hash)
           for c in range(nc)]
    pairs = []
    for i in range(nc):
        for j in range(i + 1, nc):
            s = int(shared[i][j])
            jb = jaccard_bits(bits[i], bits[j], s)
            if jb >= t:
                pairs.append((names[i], names[j], s, jb, jaccard_kmers(bits[i], bits[j], s, float(m), float(n_hash))))
    return acc, pairs


def read_tsv(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


TOL = 1.5e-6   # one unit of the last printed digit plus the rounding of log / pow between libm and numpy


def check_reports(prefix, acc, pairs):
    got = read_tsv(prefix + "_accessions.tsv", "accession\tn_ref_kmers\tbits\tfill\tfp_stated\tfp_measured")
    assert len(got) == len(acc)
    for g, w in zip(got, acc):
        assert (g[0], int(g[1]), int(g[2])) == w[:3], (g, w)
        for gv, wv in zip(g[3:], w[3:]):
            assert abs(float(gv) - wv) <= TOL, (g, w)
    got = read_tsv(prefix + "_pairs.tsv", "a\tb\tshared\tjaccard_bits\tjaccard_kmers")
    assert [(g[0], g[1], int(g[2])) for g in got] == [w[:3] for w in pairs]
    for g, w in zip(got, pairs):
        assert abs(float(g[3]) - w[3]) <= TOL, (g, w)
        if w[4] is None:
            assert g[4] == "nan", (g, w)
        else:
            assert g[4] != "nan" and abs(float(g[4]) - w[4]) <= TOL, (g, w)


# ---------------------------------------------------------------------------------------------- 5. real genomes (test.sh's parameters)

@pytest.mark.parametrize("mini", [False, True])
def test_compare_of_the_phage_build(orc, tmp_path, mini):
    tsv = tmp_path / "refs.tsv"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in PHAGES))
    suffix = ".mxi" if mini else ".bxi"
    run("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(tmp_path / "all"), "-r", str(tsv), *(("-m", "-v", "15") if mini else ()))
    oix = orc.Index.build_single_mini(str(tsv), 750000, 4, 27, 15) if mini else orc.Index.build_single(str(tsv), 750000, 4, 27)
    names, n_ref = oix.colors(), oix.n_ref_kmers()
    assert names == sorted(PHAGES)
    shared = gram(oix.rows(), 4)
    n_rows = int(oix.rows().any(axis=1).sum())
    prefix = str(tmp_path / "cmp")
    out, err = run("compare", "-i", str(tmp_path / ("all" + suffix)), "-o", prefix, "-d", "0.5")
    dups = greedy_duplicates(shared, 0.5)
    assert out.splitlines() == [f" Input index : {tmp_path / ('all' + suffix)}", "K-mer size: 27",
                                "Bloom filter parameters: num hashes 4, filter size 750000",
                                *(["Build with minimizers, minimizer size: 15"] if mini else []),
                                f"Accessions: 4, rows: {n_rows}", "Pairs reported: 6 of 6", f"Duplicates: {len(dups)} of 4 accessions"]
    assert f"Comparing 4 accessions of {tmp_path / ('all' + suffix)}" in err
    acc, pairs = expected_reports(shared, names, n_ref, 750000, 4)
    assert len(pairs) == 6
    check_reports(prefix, acc, pairs)
    assert open(prefix + "_duplicates.txt").read() == "".join(names[j] + "\n" for j in dups)


# ---------------------------------------------------------------------------------------------- 6. synthetic, planted structure

def planted_index(orc, rng, tmp_path, m=5000, nc=70, n_hash=3, m_size=0):
    """random columns; 10 and 68 exact copies of 3 (68 in the next 64-colour block), 20 = 5 with a few bits cleared, 41 = 40 with a few
    bits cleared, 30 empty, 50 saturated (every union with it is the whole filter)"""
    bits = rng.random((m, nc)) < 0.3
    bits[:, 10] = bits[:, 3]
    bits[:, 68] = bits[:, 3]
    bits[:, 20] = bits[:, 5]
    bits[rng.choice(np.flatnonzero(bits[:, 5]), size=7, replace=False), 20] = False
    bits[:, 41] = bits[:, 40]
    bits[rng.choice(np.flatnonzero(bits[:, 40]), size=150, replace=False), 41] = False
    bits[:, 30] = False
    bits[:, 50] = True
    oix = orc.Index(m, n_hash, 21, nc)
    if m_size:
        oix.set_minimizer(m_size)
    packed = np.zeros((m, oix.w32 * 32), bool)
    packed[:, :nc] = bits
    oix.rows()[:] = np.packbits(packed, axis=1, bitorder="little").view(np.uint32)
    names = random_names(rng, nc)
    n_ref = rng.integers(1, 10**5, size=nc)
    for c in range(nc):
        oix.set_color(c, names[c], int(n_ref[c]))
    path = str(tmp_path / ("planted" + (".mxi" if m_size else ".bxi")))
    oix.save(path)
    return path, gram(oix.rows(), nc), names, n_ref


def between_two_values(values, frac):
    """a threshold strictly between two neighbouring occurring values, about `frac` of the way up"""
    v = np.unique(np.asarray(values))
    k = min(max(int(len(v) * frac), 1), len(v) - 1)
    t = (v[k - 1] + v[k]) / 2
    assert v[k - 1] < t < v[k]
    return float(t)


def test_thresholds_and_duplicates_on_planted_structure(orc, tmp_path):
    rng = np.random.default_rng(19)
    m, nc, n_hash = 5000, 70, 3
    path, shared, names, n_ref = planted_index(orc, rng, tmp_path, m, nc, n_hash)
    prefix = str(tmp_path / "cmp")
    acc, all_pairs = expected_reports(shared, names, n_ref, m, n_hash)
    assert len(all_pairs) == nc * (nc - 1) // 2
    assert sum(p[4] is None for p in all_pairs) == nc - 1              # the saturated column's pairs hit the `nan` rule
    assert sum(p[3] == 1.0 for p in all_pairs) == 3                    # 3 = 10 = 68
    out, _ = run("compare", "-i", path, "-o", prefix)                  # -t defaults to 0: every pair
    assert out.splitlines()[-2:] == [f"Accessions: {nc}, rows: {m}", f"Pairs reported: {len(all_pairs)} of {len(all_pairs)}"]
    check_reports(prefix, acc, all_pairs)
    assert not os.path.exists(prefix + "_duplicates.txt")
    for frac in (0.5, 0.97):
        t = between_two_values([p[3] for p in all_pairs], frac)
        want = [p for p in all_pairs if p[3] >= t]
        assert 0 < len(want) < len(all_pairs)
        out, _ = run("compare", "-i", path, "-o", prefix, "-t", repr(t))
        assert out.splitlines()[-1] == f"Pairs reported: {len(want)} of {len(all_pairs)}"
        check_reports(prefix, acc, want)
    out, _ = run("compare", "-i", path, "-o", prefix, "-t", "1.0")     # exact copies only
    check_reports(prefix, acc, [p for p in all_pairs if p[3] == 1.0])
    assert out.splitlines()[-1] == f"Pairs reported: 3 of {len(all_pairs)}"
    # -d: the near copy 20 of 5 (7 bits cleared, 0.995) joins the exact copies; 41 (150 bits cleared of ~1500: 0.9) joins below that
    for d, want_dups in ((1.0, [10, 68]), (0.95, [10, 20, 68]), (0.85, [10, 20, 41, 68])):
        assert greedy_duplicates(shared, d) == want_dups
        out, _ = run("compare", "-i", path, "-o", prefix, "-d", repr(d), "-t", "1")
        assert out.splitlines()[-1] == f"Duplicates: {len(want_dups)} of {nc} accessions"
        assert open(prefix + "_duplicates.txt").read() == "".join(names[j] + "\n" for j in want_dups)
    # nothing reaches the threshold between unrelated columns: an empty, valid list
    sub = str(tmp_path / "few")
    keep = tmp_path / "keep.txt"
    keep.write_text("".join(names[c] + "\n" for c in (1, 2, 4)))
    run("subset", "-b", sub, "-i", path, "-a", str(keep))
    out, _ = run("compare", "-i", sub + ".bxi", "-o", prefix, "-d", "0.9")
    assert out.splitlines()[-1] == "Duplicates: 0 of 3 accessions" and open(prefix + "_duplicates.txt").read() == ""


# ---------------------------------------------------------------------------------------------- 7. round trip with subset

@pytest.mark.parametrize("m_size", [0, 11])
def test_dropping_the_duplicates_leaves_none(orc, tmp_path, m_size):
    rng = np.random.default_rng(23 + m_size)
    path, shared, names, _ = planted_index(orc, rng, tmp_path, m_size=m_size)
    suffix = ".mxi" if m_size else ".bxi"
    first, second = str(tmp_path / "first"), str(tmp_path / "second")
    out, _ = run("compare", "-i", path, "-o", first, "-d", "0.95")
    assert out.splitlines()[-1] == "Duplicates: 3 of 70 accessions"
    run("subset", "-b", str(tmp_path / "clean"), "-i", path, "-x", first + "_duplicates.txt")
    out, _ = run("compare", "-i", str(tmp_path / ("clean" + suffix)), "-o", second, "-d", "0.95")
    assert out.splitlines()[-2:] == [f"Pairs reported: {67 * 66 // 2} of {67 * 66 // 2}", "Duplicates: 0 of 67 accessions"]
    assert open(second + "_duplicates.txt").read() == ""
    gone = set(open(first + "_duplicates.txt").read().split("\n")[:-1])
    assert gone == {names[10], names[20], names[68]}
    survivors = [ln for ln in open(first + "_pairs.tsv").read().split("\n")[1:-1] if not (set(ln.split("\t")[:2]) & gone)]
    assert open(second + "_pairs.tsv").read().split("\n")[1:-1] == survivors
    acc_survivors = [ln for ln in open(first + "_accessions.tsv").read().split("\n")[1:-1] if ln.split("\t")[0] not in gone]
    assert open(second + "_accessions.tsv").read().split("\n")[1:-1] == acc_survivors


# ---------------------------------------------------------------------------------------------- 8. full size

@pytest.mark.timeout(1800)
def test_full_size_compare(tmp_path):
    """the metric's shape (m = 50 M, n = 4, k = 31, 256 colours, a fifth of the rows zero) through the CLI: the 256 x 256 matrix read back
    from the reports (bits from _accessions.tsv, shared from _pairs.tsv at -t 0) equals numpy's, exactly"""
    import torch
    from test_gpu_subset import full_size_input
    m, nc = 50_000_000, 256
    need = 4 << 30       # the counters (512 KiB) and one 256 MiB upload chunk: well under 4 GiB
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        print(f"test_full_size_compare: skipped, the device has {free >> 20} MiB free, the case needs {need >> 20} MiB")
        pytest.skip(f"device memory: {free >> 20} MiB free, {need >> 20} MiB needed")
    src, rows, names, _ = full_size_input(tmp_path, np.random.default_rng(41), m, nc)
    prefix = str(tmp_path / "cmp")
    out, _ = run("compare", "-i", src, "-o", prefix, "-t", "0")
    n_rows = header_bytes(src)[1]
    assert out.splitlines()[-2:] == [f"Accessions: {nc}, rows: {n_rows}", f"Pairs reported: {nc * (nc - 1) // 2} of {nc * (nc - 1) // 2}"]
    want = gram(rows, nc)
    got = np.zeros((nc, nc), np.uint64)
    acc = read_tsv(prefix + "_accessions.tsv", "accession\tn_ref_kmers\tbits\tfill\tfp_stated\tfp_measured")
    assert [a[0] for a in acc] == names and [int(a[1]) for a in acc] == [1000 + c for c in range(nc)]
    col = {n: c for c, n in enumerate(names)}
    for c, a in enumerate(acc):
        got[c, c] = int(a[2])
    pairs = read_tsv(prefix + "_pairs.tsv", "a\tb\tshared\tjaccard_bits\tjaccard_kmers")
    assert [(col[p[0]], col[p[1]]) for p in pairs] == [(i, j) for i in range(nc) for j in range(i + 1, nc)]
    for p in pairs:
        got[col[p[0]], col[p[1]]] = got[col[p[1]], col[p[0]]] = int(p[2])
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
