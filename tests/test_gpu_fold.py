"""`colorid fold`, cid_index_put_records_folded and cid_index_put_index_folded on the GPU.  The contract: folding an index to a Bloom size
that divides its own gives the file `build -s` writes at that size, byte for byte — checked on the four phages of test.sh (factors 2, 3,
5 and 16, .bxi and .mxi), on synthetic indices whose expected file the oracle saves from the rows OR-ed in numpy (colour counts around
the borders of 32-bit words up to more than 8192, factors from 2 to the Bloom size itself, dense and sparse rows, records in file order
and shuffled, thousands of records on one output row), chunk by chunk through the ABI in several splits and orders, on round trips with
`merge` and `subset`, and on one full-size case at the metric's shape read back in row chunks."""
import os
import struct
import subprocess

import numpy as np
import pytest

import colorid_amd
from colorid_amd import CidError
from test_gpu_merge import header_bytes, random_names, records_of, shuffle_records
from test_gpu_subset import names_of, write_list
from util import random_index

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.environ.get("COLORID_BIN", os.path.join(ROOT, "colorid_amd", "bin", "colorid"))
REFS = os.path.join(HERE, "golden", "refs")
BANNER = "\n ************** initializing logger *****************\n\n"
B021, B051, B056, B545 = (f"Listeria_phage_{n}" for n in ("B021", "B051", "B056", "B545"))


def run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.startswith(BANNER)
    return p.stdout[len(BANNER):], p.stderr


def read(path):
    with open(path, "rb") as f:
        return f.read()


def fold_rows(rows, f):
    """rows (m x w32) OR-ed over r % (m / f)"""
    m, w32 = rows.shape
    return np.bitwise_or.reduce(rows.reshape(f, m // f, w32), axis=0)


# ---------------------------------------------------------------------------------------------- real genomes (test.sh's parameters)

SIZES = {1: 750000, 2: 375000, 3: 250000, 5: 150000, 16: 46875}
ALL = [B021, B051, B056, B545]


@pytest.fixture(scope="module")
def phage_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold_phages")
    tsv = d / "all.tsv"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in ALL))
    for size in SIZES.values():
        run("build", "-s", str(size), "-n", "4", "-k", "27", "-b", str(d / f"s{size}"), "-r", str(tsv))
        run("build", "-s", str(size), "-n", "4", "-k", "27", "-b", str(d / f"s{size}_m"), "-r", str(tsv), "-m", "-v", "15")
    return d


@pytest.mark.parametrize("factor", [2, 3, 5, 16])
@pytest.mark.parametrize("flag", ["-s", "-f"])
def test_fold_of_a_build_is_the_build_at_the_smaller_size(phage_builds, factor, flag):
    d = phage_builds
    src, new = d / "s750000.bxi", SIZES[factor]
    out, err = run("fold", "-b", str(d / "got"), "-i", str(src), flag, str(new if flag == "-s" else factor))
    assert read(d / "got.bxi") == read(d / f"s{new}.bxi")
    assert out.splitlines() == [f" Input index : {src}", f" Bigsi file : {d / 'got.bxi'}", "K-mer size: 27",
                                f"Bloom filter parameters: num hashes 4, filter size {new}",
                                f"Filter size: {new} of 750000 (factor {factor})", "Saving BIGSI to file."]
    n_rows = header_bytes(str(src))[1]
    assert f"Folding {src}: {n_rows} rows into {new}\n" in err


@pytest.mark.parametrize("factor", [2, 3, 5, 16])
@pytest.mark.parametrize("flag", ["-s", "-f"])
def test_fold_of_a_minimizer_build(phage_builds, factor, flag):
    d = phage_builds
    src, new = d / "s750000_m.mxi", SIZES[factor]
    out, _ = run("fold", "-b", str(d / "got_m"), "-i", str(src), flag, str(new if flag == "-s" else factor))
    assert read(d / "got_m.mxi") == read(d / f"s{new}_m.mxi")
    assert out.splitlines() == [f" Input index : {src}", f" Bigsi file : {d / 'got_m.mxi'}", "K-mer size: 27",
                                f"Bloom filter parameters: num hashes 4, filter size {new}", "Build with minimizers, minimizer size: 15",
                                f"Filter size: {new} of 750000 (factor {factor})", "Saving BIGSI to file."]


def test_folding_in_two_steps_is_folding_once(phage_builds):
    d = phage_builds
    for suffix, m in ((".bxi", ""), (".mxi", "_m")):
        run("fold", "-b", str(d / f"half{m}"), "-i", str(d / f"s750000{m}{suffix}"), "-f", "2")
        assert read(d / f"half{m}{suffix}") == read(d / f"s375000{m}{suffix}")
        run("fold", "-b", str(d / f"sixteenth{m}"), "-i", str(d / f"half{m}{suffix}"), "-f", "8")
        assert read(d / f"sixteenth{m}{suffix}") == read(d / f"s46875{m}{suffix}")


def test_factor_1_reproduces_the_input(phage_builds):
    d = phage_builds
    out, _ = run("fold", "-b", str(d / "same"), "-i", str(d / "s750000.bxi"), "-s", "750000")
    assert read(d / "same.bxi") == read(d / "s750000.bxi")
    assert "Filter size: 750000 of 750000 (factor 1)" in out
    run("fold", "-b", str(d / "same_m"), "-i", str(d / "s46875_m.mxi"), "-f", "1")
    assert read(d / "same_m.mxi") == read(d / "s46875_m.mxi")


def test_fold_by_false_positive_bound(phage_builds):
    """-p picks a divisor; whichever it picks, the file is the fold to that size — here a bound that only the sizes 750000 and 375000
    of the built ones meet, so the choice can be compared with a build"""
    d = phage_builds
    out, _ = run("info", "-b", str(d / "s375000.bxi"))
    worst_375 = max(float(ln.split()[2]) for ln in out.splitlines() if ln.startswith("Listeria"))
    out, _ = run("info", "-b", str(d / "s250000.bxi"))
    worst_250 = max(float(ln.split()[2]) for ln in out.splitlines() if ln.startswith("Listeria"))
    assert worst_375 < worst_250
    bound = (worst_375 + worst_250) / 2
    out, _ = run("fold", "-b", str(d / "by_p"), "-i", str(d / "s750000.bxi"), "-p", f"{bound:.6f}")
    size = int(out.split("Filter size: ")[1].split()[0])
    assert 250000 < size <= 375000 and 750000 % size == 0
    run("fold", "-b", str(d / "by_s"), "-i", str(d / "s750000.bxi"), "-s", str(size))
    assert read(d / "by_p.bxi") == read(d / "by_s.bxi")
    if size == 375000:
        assert read(d / "by_p.bxi") == read(d / "s375000.bxi")


# ---------------------------------------------------------------------------------------------- synthetic, composed by the oracle

def name_and_save(orc, rng, tmp_path, src, f, m_size=0, shuffle=False, stem=""):
    """names the colours of the oracle index `src`, writes it and the expected fold by f (rows OR-ed in numpy, saved by the oracle)"""
    nc, m = src.n_colors, src.m
    suffix = ".mxi" if m_size else ".bxi"
    names = random_names(rng, nc)
    n_ref = rng.integers(0, 10**9, size=nc)
    exp = orc.Index(m // f, src.n_hash, src.k, nc)
    for ix in (src, exp):
        for c in range(nc):
            ix.set_color(c, names[c], int(n_ref[c]))
        if m_size:
            ix.set_minimizer(m_size)
    exp.rows()[:] = fold_rows(src.rows(), f)
    src_path, want = str(tmp_path / f"in{stem}{suffix}"), str(tmp_path / f"want{stem}{suffix}")
    src.save(src_path)
    exp.save(want)
    if shuffle:
        shuffle_records(src_path, rng)
    return src_path, want


def compose_fold(orc, rng, tmp_path, nc, m, f, m_size=0, shuffle=False, density=0.3, zero_row_frac=0.3):
    src = random_index(orc, rng, m, 3, 21, nc, density=density, zero_row_frac=zero_row_frac)
    return name_and_save(orc, rng, tmp_path, src, f, m_size=m_size, shuffle=shuffle)


WIDTHS = (1, 31, 32, 33, 64, 257, 8300)


def factors_of(nc):
    m = 300 if nc > 8192 else 600
    return [(m, f) for f in (2, 3, 12, m // 4, m)]


@pytest.mark.parametrize("nc,m,f", [(nc, m, f) for nc in WIDTHS for m, f in factors_of(nc)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_fold_matches_oracle_composed_index(orc, tmp_path, nc, m, f, shuffle):
    rng = np.random.default_rng(nc * 131 + f * 2 + shuffle)
    # few enough bits that f rows OR-ed together are neither empty nor full
    src, want = compose_fold(orc, rng, tmp_path, nc, m, f, shuffle=shuffle, density=min(0.3, 1.5 / f), zero_row_frac=0.3)
    run("fold", "-b", str(tmp_path / "got"), "-i", src, "-f", str(f))
    assert read(tmp_path / "got.bxi") == read(want)


@pytest.mark.parametrize("density,zero_row_frac", [(0.9, 0.0), (0.5, 0.2), (0.002, 0.0), (0.3, 0.95), (0.0005, 0.9)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_dense_sparse_and_mostly_absent_rows(orc, tmp_path, density, zero_row_frac, shuffle):
    rng = np.random.default_rng(int(density * 1e4) + shuffle)
    src, want = compose_fold(orc, rng, tmp_path, 100, 3000, 6, shuffle=shuffle, density=density, zero_row_frac=zero_row_frac)
    run("fold", "-b", str(tmp_path / "got"), "-i", src, "-s", "500")
    assert read(tmp_path / "got.bxi") == read(want)
    if density < 0.001:
        assert header_bytes(str(tmp_path / "got.bxi"))[1] < 500    # output rows that no input row reaches are not written


def test_fold_matches_oracle_composed_minimizer_index(orc, tmp_path):
    rng = np.random.default_rng(7)
    src, want = compose_fold(orc, rng, tmp_path, 65, 600, 4, m_size=11, shuffle=True, density=0.1)
    run("fold", "-b", str(tmp_path / "got"), "-i", src, "-f", "4")
    assert read(tmp_path / "got.mxi") == read(want)


def graded_index(orc, rng, m, nc):
    """columns from nearly empty to a third full, so that a fold by thousands leaves some colours sparse and fills others"""
    ix = orc.Index(m, 3, 21, nc)
    dens = np.logspace(-7.5, -0.5, nc)
    bits = np.zeros((m, ix.w32 * 32), bool)
    bits[:, :nc] = rng.random((m, nc)) < dens[None, :]
    ix.rows()[:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint32)
    return ix


@pytest.mark.parametrize("m,m_new", [(200_000, 8), (200_000, 1), (196_608, 3)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_thousands_of_records_on_one_output_row(orc, tmp_path, m, m_new, shuffle):
    """one piece, one launch: every output row takes the OR of tens of thousands of records, in file order and shuffled"""
    rng = np.random.default_rng(m_new + shuffle)
    src = graded_index(orc, rng, m, 40)
    n_records = int(src.rows().any(axis=1).sum())
    assert n_records // m_new > 5000
    folded = fold_rows(src.rows(), m // m_new)
    fill = np.unpackbits(folded.view(np.uint8), bitorder="little").sum() / (m_new * 40)
    assert 0.05 < fill < 0.95, fill
    src_path, want = name_and_save(orc, rng, tmp_path, src, m // m_new, shuffle=shuffle)
    run("fold", "-b", str(tmp_path / "got"), "-i", src_path, "-s", str(m_new))
    assert read(tmp_path / "got.bxi") == read(want)


# ---------------------------------------------------------------------------------------------- the ABI calls

def dense_records(rows, nc, order=None):
    """the non-zero rows of a dense u32 matrix as .bxi records, in `order` (row ids) or ascending"""
    w32 = rows.shape[1]
    nz = np.flatnonzero(rows.any(axis=1)) if order is None else np.asarray(order)
    out = np.empty(len(nz), np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (w32,)), ("nb", "<u8")]))
    out["row"], out["nw"], out["w"], out["nb"] = nz, w32, rows[nz], nc
    return out.tobytes()


@pytest.mark.parametrize("nc", [1, 33, 64, 257])
@pytest.mark.parametrize("f", [1, 2, 7, 210])
def test_put_records_folded_and_put_index_folded_give_the_numpy_fold(orc, hip_ctx, nc, f):
    rng = np.random.default_rng(nc * 1000 + f)
    m = 2100
    oix = random_index(orc, rng, m, 3, 21, nc, density=min(0.3, 0.7 / f), zero_row_frac=0.25)
    want = fold_rows(oix.rows(), f)
    assert want.any() and not (want[:, 0] & 1).all()
    a = colorid_amd.Index(hip_ctx, m // f, 3, 21, nc)
    a.put_records_folded(dense_records(oix.rows(), nc), m)
    a.finalize()
    src = colorid_amd.Index(hip_ctx, m, 3, 21, nc)
    src.put_dense(oix.rows())
    src.finalize()
    b = colorid_amd.Index(hip_ctx, m // f, 3, 21, nc)
    b.put_index_folded(src)
    b.finalize()
    every = list(range(m // f))
    assert np.array_equal(a.get_rows(every), want)
    assert np.array_equal(b.get_rows(every), want)
    for ix in (a, b, src):
        ix.close()


def test_put_index_folded_over_wide_rows_and_a_single_output_row(orc, hip_ctx):
    """more than 8192 colours (the wide row stride), and m' = 1: the slices of the source are taken in chunks that share the output row"""
    rng = np.random.default_rng(12)
    for nc, m, f, density in ((8300, 300, 5, 0.1), (70, 60000, 60000, 1e-5), (70, 60000, 30000, 2e-5)):
        oix = random_index(orc, rng, m, 3, 21, nc, density=density, zero_row_frac=0.1)
        want = fold_rows(oix.rows(), f)
        bits = np.unpackbits(want.view(np.uint8), bitorder="little").sum()
        assert 0 < bits < (m // f) * nc
        src = colorid_amd.Index(hip_ctx, m, 3, 21, nc)
        src.put_dense(oix.rows())
        src.finalize()
        dst = colorid_amd.Index(hip_ctx, m // f, 3, 21, nc)
        dst.put_index_folded(src)
        dst.finalize()
        assert np.array_equal(dst.get_rows(list(range(m // f))), want)
        dst.close()
        src.close()


def test_both_calls_or_into_what_is_there(hip_ctx):
    """OR-ed, not stored: a row put again keeps its bits; the two forms and a plain put mix"""
    ix = colorid_amd.Index(hip_ctx, 10, 2, 21, 4)
    ix.put_records(records_of({3: [0b0001]}, 4))
    ix.put_records_folded(records_of({3: [0b0010], 13: [0b0100], 29: [0b0001]}, 4), 30)
    ix.put_records_folded(records_of({3: [0b1000]}, 4), 10)                   # factor 1: a plain OR-put
    src = colorid_amd.Index(hip_ctx, 20, 2, 21, 4)
    src.put_records(records_of({19: [0b0100], 4: [0b0001]}, 4))
    src.finalize()
    ix.put_index_folded(src)
    ix.finalize()
    assert ix.get_rows([3, 4, 9, 0]).tolist() == [[0b1111], [0b0001], [0b0101], [0]]
    ix.close()
    src.close()


def test_chunks_in_any_split_and_order_give_one_index(orc, hip_ctx):
    """the upload-chunk switch of the library is the search's (stage_records cuts its pieces at 256 MiB whatever it says), so the pieces
    are made here: the records of one file through the ABI in several splits and orders"""
    rng = np.random.default_rng(99)
    m, f, nc = 6000, 12, 90
    oix = random_index(orc, rng, m, 3, 21, nc, density=0.05, zero_row_frac=0.3)
    want = fold_rows(oix.rows(), f)
    nz = np.flatnonzero(oix.rows().any(axis=1))
    every = list(range(m // f))
    for split in ([len(nz)], [1, len(nz) - 1], [len(nz) // 2] * 2 + [len(nz) % 2], [7] * (len(nz) // 7) + [len(nz) % 7], [0, len(nz), 0]):
        for order in ("file", "reversed", "shuffled"):
            rows = {"file": nz, "reversed": nz[::-1], "shuffled": rng.permutation(nz)}[order]
            chunks = np.split(rows, np.cumsum(split)[:-1])
            if order == "shuffled":
                chunks = [chunks[i] for i in rng.permutation(len(chunks))]
            ix = colorid_amd.Index(hip_ctx, m // f, 3, 21, nc)
            for ch in chunks:
                ix.put_records_folded(dense_records(oix.rows(), nc, ch), m)
            ix.finalize()
            assert np.array_equal(ix.get_rows(every), want), (split[:3], order)
            ix.close()


def test_put_records_folded_refusals(hip_ctx):
    ix = colorid_amd.Index(hip_ctx, 100, 2, 21, 3)
    rec = records_of({5: [0b101]}, 3)
    with pytest.raises(CidError) as e:                                           # a file of no rows
        ix.put_records_folded(rec, 0)
    assert e.value.code == -1 and "not a multiple" in str(e.value)
    for bad in (150, 99, 50, 1):                                                 # not a multiple of the index's 100
        with pytest.raises(CidError) as e:
            ix.put_records_folded(rec, bad)
        assert e.value.code == -1 and f"bloom_size {bad} does not fold onto 100 rows" in str(e.value)
    assert ix.lib.cid_index_put_records_folded(None, None, 0, 100) == -1         # null arguments
    assert ix.lib.cid_index_put_records_folded(ix.h, None, 1, 100) == -1
    # malformed records, with cid_index_put_records' text
    with pytest.raises(CidError) as e:                                           # two words announced, the file's shape has one
        ix.put_records_folded(struct.pack("<QQIQ", 5, 2, 0b101, 3), 200)
    assert e.value.code == -1 and "word count != ceil(n_colors/32)" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit count that is not the file's
        ix.put_records_folded(records_of({5: [0b101]}, 4), 200)
    assert e.value.code == -1 and "bit count != n_colors" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit past the 3 colours
        ix.put_records_folded(records_of({5: [0b1101]}, 3), 200)
    assert e.value.code == -1 and "bits beyond n_colors" in str(e.value)
    # a row at or past the FILE's size is refused although row % 100 is a row of the index — and the good record beside it is not applied
    for row in (200, 205, 2**32 + 5, 2**63 + 5):
        with pytest.raises(CidError) as e:
            ix.put_records_folded(records_of({7: [0b011], row: [0b101]}, 3), 200)
        assert e.value.code == -1 and "row >= bloom_size" in str(e.value)
    ix.put_records_folded(records_of({199: [0b110]}, 3), 200)                    # the last row of the file is one
    ix.put_records_folded(rec, 200)
    ix.finalize()
    assert ix.get_rows([5, 7, 99, 0]).tolist() == [[0b101], [0], [0b110], [0]]
    with pytest.raises(CidError) as e:
        ix.put_records_folded(rec, 200)
    assert e.value.code == -5
    ix.close()


def test_put_index_folded_refusals(hip_ctx):
    dst = colorid_amd.Index(hip_ctx, 100, 2, 21, 3)
    src = colorid_amd.Index(hip_ctx, 200, 2, 21, 3)
    src.put_records(records_of({105: [0b101]}, 3))
    assert dst.lib.cid_index_put_index_folded(None, src.h) == -1 and dst.lib.cid_index_put_index_folded(dst.h, None) == -1
    with pytest.raises(CidError) as e:                                           # the source is still being filled
        dst.put_index_folded(src)
    assert e.value.code == -1 and "not finalized" in str(e.value)
    src.finalize()
    for m, nc, text in ((200, 4, "4 colours into an index of 3"), (150, 3, "bloom_size 150 does not fold onto 100 rows"),
                        (50, 3, "bloom_size 50 does not fold onto 100 rows")):
        other = colorid_amd.Index(hip_ctx, m, 2, 21, nc).finalize()
        with pytest.raises(CidError) as e:
            dst.put_index_folded(other)
        assert e.value.code == -1 and text in str(e.value)
        other.close()
    dst.put_index_folded(src)
    dst.finalize()
    assert dst.get_rows([5, 6]).tolist() == [[0b101], [0]]
    with pytest.raises(CidError) as e:
        dst.put_index_folded(src)
    assert e.value.code == -5
    dst.close()
    src.close()


def test_put_index_folded_refuses_another_device():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: an index on another device cannot be made")
    c0, c1 = colorid_amd.Context(0), colorid_amd.Context(1)
    dst = colorid_amd.Index(c0, 100, 2, 21, 3)
    src = colorid_amd.Index(c1, 200, 2, 21, 3).finalize()
    with pytest.raises(CidError) as e:
        dst.put_index_folded(src)
    assert e.value.code == -1 and "device" in str(e.value)
    for x in (dst, src, c0, c1):
        x.close()


def test_a_malformed_record_in_a_later_piece_is_refused_and_the_piece_left_out(hip_ctx):
    """more than 256 MiB of records in one call: the first piece is applied, the second — one bad record near its end — is refused as a
    whole and names the fault; the index holds the first piece and nothing of the second"""
    rng = np.random.default_rng(3)
    m_file, m, nc = 1 << 24, 1 << 12, 20
    n = 10_500_000                                                                # x 28 bytes = 294 MB: two pieces
    per_piece = (256 << 20) // 28
    assert per_piece < n - 1000
    recs = np.empty(n, np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (1,)), ("nb", "<u8")]))
    recs["row"] = rng.integers(0, m_file, size=n)
    recs["nw"], recs["nb"] = 1, nc
    recs["w"][:, 0] = 1 << rng.integers(0, nc, size=n).astype(np.uint32)
    recs["w"][rng.random(n) < 0.9, 0] = 0                                         # most words zero: the folded rows stay part-filled
    recs["nb"][n - 5] = nc + 1
    ix = colorid_amd.Index(hip_ctx, m, 2, 21, nc)
    with pytest.raises(CidError) as e:
        ix.put_records_folded(recs.tobytes(), m_file)
    assert e.value.code == -1 and "bit count != n_colors" in str(e.value)
    ix.finalize()
    want = np.zeros(m, np.uint32)
    np.bitwise_or.at(want, (recs["row"][:per_piece] % m).astype(np.int64), recs["w"][:per_piece, 0])
    got = ix.get_rows(list(range(m)))[:, 0]
    assert 0 < np.unpackbits(want.view(np.uint8)).sum() < m * nc
    assert np.array_equal(got, want)
    ix.close()


# ---------------------------------------------------------------------------------------------- round trips with merge and subset

def test_fold_then_merge_of_builds_at_different_sizes(phage_builds):
    """two collections built at different sizes, brought to the smaller one and merged: the build over the union at that size"""
    d = phage_builds
    for name, accs, size in (("ab", [B021, B056], 750000), ("cd", [B051, B545], 375000)):
        tsv = d / f"{name}.tsv"
        tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in accs))
        run("build", "-s", str(size), "-n", "4", "-k", "27", "-b", str(d / name), "-r", str(tsv))
    p = subprocess.run([BIN, "merge", "-b", str(d / "no"), "-i", str(d / "ab.bxi"), str(d / "cd.bxi")], capture_output=True, text=True)
    assert p.returncode != 0 and "bloom_size differs" in p.stderr                # merge keeps refusing unequal sizes
    run("fold", "-b", str(d / "ab_half"), "-i", str(d / "ab.bxi"), "-s", "375000")
    run("merge", "-b", str(d / "abcd"), "-i", str(d / "ab_half.bxi"), str(d / "cd.bxi"))
    assert read(d / "abcd.bxi") == read(d / "s375000.bxi")


@pytest.mark.parametrize("nc,f,shuffle", [(64, 4, False), (257, 10, True), (1000, 3, True)])
def test_subset_then_fold_is_fold_then_subset(orc, tmp_path, nc, f, shuffle):
    rng = np.random.default_rng(nc + f)
    src, _ = compose_fold(orc, rng, tmp_path, nc, 600, f, shuffle=shuffle, density=0.08)
    names = names_of(src)
    keep = write_list(tmp_path / "keep.txt", [n for n in names if rng.random() < 0.4] or names[:1])
    run("subset", "-b", str(tmp_path / "s"), "-i", src, "-a", keep)
    run("fold", "-b", str(tmp_path / "sf"), "-i", str(tmp_path / "s.bxi"), "-f", str(f))
    run("fold", "-b", str(tmp_path / "f"), "-i", src, "-f", str(f))
    run("subset", "-b", str(tmp_path / "fs"), "-i", str(tmp_path / "f.bxi"), "-a", keep)
    assert read(tmp_path / "sf.bxi") == read(tmp_path / "fs.bxi")
    assert header_bytes(str(tmp_path / "sf.bxi"))[1] > 0


# ---------------------------------------------------------------------------------------------- behaviour of the folded index

def test_search_and_read_id_on_the_folded_index(phage_builds):
    d = phage_builds
    run("fold", "-b", str(d / "f5"), "-i", str(d / "s750000.bxi"), "-f", "5")
    q = os.path.join(REFS, B051 + ".fasta")
    outs = [run("search", "-b", str(d / f"{stem}.bxi"), "-q", q, "-s")[0] for stem in ("f5", "s150000")]
    assert outs[0] == outs[1] and B051 in outs[0]
    for stem in ("f5", "s150000"):
        run("read_id", "-b", str(d / f"{stem}.bxi"), "-q", q, "-n", str(d / f"rid_{stem}"), "-B", "0")
    for part in ("_reads.txt", "_counts.txt"):
        assert read(d / f"rid_f5{part}") == read(d / f"rid_s150000{part}")
    assert len(read(d / "rid_f5_reads.txt")) > 0


def test_compare_counts_the_folded_columns(orc, tmp_path):
    rng = np.random.default_rng(21)
    nc, m, f = 70, 3000, 6
    oix = random_index(orc, rng, m, 3, 21, nc, density=0.05, zero_row_frac=0.2)
    folded = fold_rows(oix.rows(), f)
    src, _ = name_and_save(orc, rng, tmp_path, oix, f)
    run("fold", "-b", str(tmp_path / "got"), "-i", src, "-f", str(f))
    run("compare", "-i", str(tmp_path / "got.bxi"), "-o", str(tmp_path / "cmp"))
    lines = open(str(tmp_path / "cmp_accessions.tsv")).read().split("\n")[1:-1]
    bits = np.unpackbits(folded.view(np.uint8), axis=1, bitorder="little")[:, :nc].sum(axis=0)
    assert [ln.split("\t")[0] for ln in lines] == names_of(src)
    assert [int(ln.split("\t")[2]) for ln in lines] == bits.tolist()
    assert 0 < bits.min() and bits.max() < m // f


# ---------------------------------------------------------------------------------------------- full size

@pytest.mark.timeout(1800)
def test_full_size_fold_of_a_resident_index():
    """the metric's shape (m = 50 M, 256 colours): a planted resident index folded by 2 and by 10 (cid_index_put_index_folded), read back
    in row chunks against the numpy OR of the source's chunks.  One bit in 16 is set, so the folds are 12 % and 48 % full"""
    import torch
    m, nc, w32 = 50_000_000, 256, 8
    need = 4 << 30       # the source (1.6 GB), the larger fold (0.8 GB), the chunks that go up and come back: well under 4 GiB
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        print(f"test_full_size_fold_of_a_resident_index: skipped, the device has {free >> 20} MiB free, the case needs {need >> 20} MiB")
        pytest.skip(f"device memory: {free >> 20} MiB free, {need >> 20} MiB needed")
    rng = np.random.default_rng(51)
    rows = rng.integers(0, 2**32, size=(m, w32), dtype=np.uint32)
    for _ in range(3):
        rows &= rng.integers(0, 2**32, size=(m, w32), dtype=np.uint32)
    rows[rng.random(m) < 0.2] = 0
    ctx = colorid_amd.Context(0)
    src = colorid_amd.Index(ctx, m, 4, 31, nc)
    step = 1 << 22
    for r0 in range(0, m, step):
        src.put_rows(np.arange(r0, min(m, r0 + step), dtype=np.uint64), rows[r0:r0 + step])
    src.finalize()
    for f in (2, 10):
        m_new = m // f
        dst = colorid_amd.Index(ctx, m_new, 4, 31, nc)
        dst.put_index_folded(src)
        dst.finalize()
        set_bits = 0
        for r0 in range(0, m_new, step):
            r1 = min(m_new, r0 + step)
            want = rows[r0:r1].copy()
            for s in range(1, f):
                want |= rows[s * m_new + r0:s * m_new + r1]
            set_bits += int(np.unpackbits(want.view(np.uint8)).sum(dtype=np.int64))
            assert np.array_equal(dst.get_rows(np.arange(r0, r1, dtype=np.uint64)), want), (f, r0)
        fill = set_bits / (m_new * nc)
        assert 0.05 < fill < 0.6, (f, fill)                                       # neither empty nor saturated
        dst.close()
    src.close()
    ctx.close()
