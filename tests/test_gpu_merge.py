"""`colorid merge` and cid_index_put_records_mapped on the GPU.  The contract: merging indices built with equal parameters gives the
file `build` writes over the union of their reference lists, byte for byte — checked on the four phages of test.sh, and on synthetic
indices whose expected file the oracle composes (columns placed by sorted accession name) for colour splits that interleave finely,
cross word boundaries and go past 8192 colours, with the inputs' records in file order and shuffled (the Rust binary writes them in
HashMap order).  One full-size case at the metric's shape is compared in row chunks."""
import os
import struct
import subprocess

import numpy as np
import pytest

import colorid_amd
from colorid_amd import CidError
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


# ---------------------------------------------------------------------------------------------- real genomes (test.sh's parameters)

@pytest.fixture(scope="module")
def phage_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_phages")
    sets = {"a": [B021, B056], "b": [B051, B545], "c": [B051], "d": [B545], "all": [B021, B051, B056, B545]}
    for name, accs in sets.items():
        tsv = d / f"{name}.tsv"
        tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in accs))
        run("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / name), "-r", str(tsv))
        run("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / f"{name}_m"), "-r", str(tsv), "-m", "-v", "15")
    return d


def test_merge_of_two_builds_is_the_union_build(phage_builds):
    d = phage_builds
    out, err = run("merge", "-b", str(d / "ab"), "-i", str(d / "a.bxi"), str(d / "b.bxi"))
    assert read(d / "ab.bxi") == read(d / "all.bxi")
    assert out.splitlines() == [f" Input indices : {d / 'a.bxi'} {d / 'b.bxi'}", f" Bigsi file : {d / 'ab.bxi'}", "K-mer size: 27",
                                "Bloom filter parameters: num hashes 4, filter size 750000", "Accessions: 4 (2 + 2)", "Saving BIGSI to file."]
    assert f"Merging {d / 'a.bxi'} into index (1/2): 2 accessions" in err and f"Merging {d / 'b.bxi'} into index (2/2)" in err
    # the order of the inputs does not matter
    run("merge", "-b", str(d / "ba"), "-i", str(d / "b.bxi"), str(d / "a.bxi"))
    assert read(d / "ba.bxi") == read(d / "all.bxi")


def test_three_way_merge_with_singletons(phage_builds):
    d = phage_builds
    run("merge", "-b", str(d / "acd"), "-i", str(d / "d.bxi"), str(d / "a.bxi"), str(d / "c.bxi"))
    assert read(d / "acd.bxi") == read(d / "all.bxi")


def test_merge_of_minimizer_indices(phage_builds):
    d = phage_builds
    out, _ = run("merge", "-b", str(d / "ab_m"), "-i", str(d / "a_m.mxi"), str(d / "b_m.mxi"))
    assert "Build with minimizers, minimizer size: 15" in out
    assert read(d / "ab_m.mxi") == read(d / "all_m.mxi")
    run("merge", "-b", str(d / "acd_m"), "-i", str(d / "a_m.mxi"), str(d / "c_m.mxi"), str(d / "d_m.mxi"))
    assert read(d / "acd_m.mxi") == read(d / "all_m.mxi")


# ---------------------------------------------------------------------------------------------- synthetic, composed by the oracle

def header_bytes(path):
    """offset of the first row record, the number of records and the record size of a .bxi/.mxi file"""
    raw = read(path)
    at = 32 if path.endswith(".mxi") else 24
    nc = struct.unpack_from("<Q", raw, at)[0]
    at += 8
    for _ in range(nc):
        n = struct.unpack_from("<Q", raw, at + 8)[0]
        at += 16 + n
    n_rows = struct.unpack_from("<Q", raw, at)[0]
    return at + 8, n_rows, 24 + 4 * ((nc + 31) // 32)


def shuffle_records(path, rng):
    start, n_rows, rec = header_bytes(path)
    raw = bytearray(read(path))
    recs = np.frombuffer(bytes(raw[start:start + n_rows * rec]), np.uint8).reshape(n_rows, rec)
    raw[start:start + n_rows * rec] = recs[rng.permutation(n_rows)].tobytes()
    with open(path, "wb") as f:
        f.write(bytes(raw))


def random_names(rng, n):
    names = set()
    while len(names) < n:
        names.add("".join(rng.choice(list("ACGTacgt_.0123456789"), size=int(rng.integers(1, 12)))))
    return sorted(names, key=lambda s: s.encode())


def compose(orc, rng, tmp_path, split, m=2000, m_size=0, shuffle=False):
    """the expected index (colours = sorted names) and one oracle-written input per part of the split, colours dealt at random"""
    total = sum(split)
    suffix = ".mxi" if m_size else ".bxi"
    exp = random_index(orc, rng, m, 3, 21, total, density=0.3, zero_row_frac=0.3)
    names = random_names(rng, total)
    n_ref = rng.integers(0, 10**9, size=total)
    for c in range(total):
        exp.set_color(c, names[c], int(n_ref[c]))
    if m_size:
        exp.set_minimizer(m_size)
    bits = np.unpackbits(exp.rows().view(np.uint8), axis=1, bitorder="little")[:, :total].astype(bool)
    owner = rng.permutation(np.repeat(np.arange(len(split)), split))
    paths = []
    for i in range(len(split)):
        cols = np.flatnonzero(owner == i)                     # ascending == in name order
        ix = orc.Index(m, 3, 21, len(cols))
        if m_size:
            ix.set_minimizer(m_size)
        packed = np.zeros((m, ix.w32 * 32), bool)
        packed[:, :len(cols)] = bits[:, cols]
        ix.rows()[:] = np.packbits(packed, axis=1, bitorder="little").view(np.uint32)
        for j, c in enumerate(cols):
            ix.set_color(j, names[c], int(n_ref[c]))
        p = str(tmp_path / f"in{i}{suffix}")
        ix.save(p)
        if shuffle:
            shuffle_records(p, rng)
        paths.append(p)
    want = str(tmp_path / f"want{suffix}")
    exp.save(want)
    return paths, want


@pytest.mark.parametrize("split", [(1, 1), (31, 33), (64, 64), (100, 157, 3), (6000, 4000)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_merge_matches_oracle_composed_index(orc, tmp_path, split, shuffle):
    rng = np.random.default_rng(sum(split) + shuffle)
    paths, want = compose(orc, rng, tmp_path, split, m=400 if sum(split) > 8192 else 2000, shuffle=shuffle)
    run("merge", "-b", str(tmp_path / "got"), "-i", *paths)
    assert read(tmp_path / "got.bxi") == read(want)


def test_merge_matches_oracle_composed_minimizer_index(orc, tmp_path):
    rng = np.random.default_rng(7)
    paths, want = compose(orc, rng, tmp_path, (40, 25), m_size=11, shuffle=True)
    run("merge", "-b", str(tmp_path / "got"), "-i", *paths)
    assert read(tmp_path / "got.mxi") == read(want)


# ---------------------------------------------------------------------------------------------- the ABI call

def records_of(words_by_row, n_colors):
    """.bxi records of {row: u32 words}"""
    w32 = (n_colors + 31) // 32
    out = b""
    for r, w in words_by_row.items():
        out += struct.pack("<QQ", r, w32) + np.asarray(w, np.uint32).tobytes() + struct.pack("<Q", n_colors)
    return out


def test_put_records_mapped_deposits_through_the_map(hip_ctx):
    ix = colorid_amd.Index(hip_ctx, 100, 2, 21, 70)
    # file colours 0..4 -> 3, 30, 31, 32, 69: runs cross output words and a file word's bits spread over three output words
    cmap = np.array([3, 30, 31, 32, 69], np.uint32)
    ix.put_records_mapped(records_of({7: [0b11110], 99: [0b00001], 0: [0]}, 5), 5, cmap)
    ix.put_records_mapped(records_of({7: [0b1]}, 1), 1, np.array([0], np.uint32))
    ix.finalize()
    got = ix.get_rows([0, 7, 99])
    assert got.tolist() == [[0, 0, 0], [(3 << 30) | 1, 1, 1 << 5], [1 << 3, 0, 0]]
    ix.close()


def test_put_records_mapped_refusals(hip_ctx):
    ix = colorid_amd.Index(hip_ctx, 100, 2, 21, 70)
    rec = records_of({5: [0b11]}, 2)
    for bad in ([4, 4], [5, 4], [0, 70]):                   # not increasing (twice), out of range
        with pytest.raises(CidError) as e:
            ix.put_records_mapped(rec, 2, np.array(bad, np.uint32))
        assert e.value.code == -1
    with pytest.raises(CidError) as e:                      # a bit past the file's 2 colours
        ix.put_records_mapped(records_of({5: [0b111]}, 2), 2, np.array([0, 1], np.uint32))
    assert e.value.code == -1 and "bits beyond n_colors" in str(e.value)
    with pytest.raises(CidError) as e:                      # a bit count that is not the file's
        ix.put_records_mapped(records_of({5: [0b11]}, 3), 2, np.array([0, 1], np.uint32))
    assert e.value.code == -1
    with pytest.raises(CidError) as e:                      # a row past bloom_size
        ix.put_records_mapped(records_of({100: [1]}, 2), 2, np.array([0, 1], np.uint32))
    assert e.value.code == -1 and "row >= bloom_size" in str(e.value)
    ix.finalize()
    with pytest.raises(CidError) as e:
        ix.put_records_mapped(rec, 2, np.array([0, 1], np.uint32))
    assert e.value.code == -5
    ix.close()


# ---------------------------------------------------------------------------------------------- full size

def write_bxi(path, m, n_hash, k, names, rows):
    """a .bxi of dense rows (m x w32 u32), written as build writes it (ascending rows, all-zero rows dropped), in chunks"""
    nc = len(names)
    w32 = rows.shape[1]
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQQ", m, n_hash, k, nc))
        for c, n in enumerate(names):
            f.write(struct.pack("<QQ", c, len(n)) + n.encode())
        count_at = f.tell()
        f.write(struct.pack("<Q", 0))
        rec = np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (w32,)), ("nb", "<u8")])
        n = 0
        for r0 in range(0, m, 1 << 22):
            blk = rows[r0:r0 + (1 << 22)]
            nz = np.flatnonzero(blk.any(axis=1))
            out = np.empty(len(nz), rec)
            out["row"], out["nw"], out["w"], out["nb"] = nz + r0, w32, blk[nz], nc
            f.write(out.tobytes())
            n += len(nz)
        f.write(struct.pack("<Q", nc))
        for c, nm in enumerate(names):
            f.write(struct.pack("<Q", len(nm)) + nm.encode() + struct.pack("<Q", 1000 + c))
        f.seek(count_at)
        f.write(struct.pack("<Q", n))


def full_size_inputs(d, rng, m=50_000_000, half=128):
    """two 128-colour halves of the metric's shape (m = 50 M, n = 4, k = 31), colours interleaved by name; returns the paths, the
    halves' rows and where each half's colours land in the merged order"""
    names = random_names(rng, 2 * half)
    owner = rng.permutation(np.repeat([0, 1], half))
    cols = [np.flatnonzero(owner == i) for i in (0, 1)]
    paths, rows = [], []
    for i in (0, 1):
        w = rng.integers(0, 2**32, size=(m, half // 32), dtype=np.uint32) & rng.integers(0, 2**32, size=(m, half // 32), dtype=np.uint32)
        w[rng.random(m) < 0.2] = 0
        p = str(d / f"half{i}.bxi")
        write_bxi(p, m, 4, 31, [names[c] for c in cols[i]], w)
        paths.append(p)
        rows.append(w)
    return paths, rows, cols, names


def check_merged(merged, m, rows, cols, names):
    """the merged file against the halves, in row chunks (never a dense bool array of the whole index)"""
    start, n_rows, rec = header_bytes(merged)
    assert rec == 24 + 4 * 8
    recs = np.memmap(merged, dtype=np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (8,)), ("nb", "<u8")]), mode="r", offset=start,
                     shape=(n_rows,))
    seen = 0
    step = 1 << 21
    for r0 in range(0, m, step):
        want = np.zeros((min(step, m - r0), 256), bool)
        for i in (0, 1):
            want[:, cols[i]] = np.unpackbits(rows[i][r0:r0 + step].view(np.uint8), axis=1, bitorder="little")
        want_w = np.packbits(want, axis=1, bitorder="little").view(np.uint32)
        nz = np.flatnonzero(want_w.any(axis=1))
        got = recs[seen:seen + len(nz)]
        assert np.array_equal(got["row"], nz + r0), r0
        assert np.array_equal(got["w"], want_w[nz]), r0
        assert (got["nw"] == 8).all() and (got["nb"] == 256).all()
        seen += len(nz)
    assert seen == n_rows
    del recs
    with open(merged, "rb") as f:
        f.seek(start + n_rows * rec)
        tail = f.read()
    by_name = {names[c]: 1000 + j for i in (0, 1) for j, c in enumerate(cols[i])}
    assert tail == struct.pack("<Q", 256) + b"".join(struct.pack("<Q", len(n)) + n.encode() + struct.pack("<Q", by_name[n]) for n in names)


@pytest.mark.timeout(1800)
def test_full_size_merge(tmp_path):
    rng = np.random.default_rng(31)
    m = 50_000_000
    paths, rows, cols, names = full_size_inputs(tmp_path, rng, m)
    run("merge", "-b", str(tmp_path / "merged"), "-i", *paths)
    check_merged(str(tmp_path / "merged.bxi"), m, rows, cols, names)
