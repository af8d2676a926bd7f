"""`colorid subset` and cid_index_put_records_subset on the GPU.  The contract: the subset of an index is the file `build` writes over
the kept lines of the reference list, byte for byte — checked on the four phages of test.sh, on synthetic indices whose expected file
the oracle saves from the kept columns re-packed in numpy (keep patterns from dense to 1 in 100, borders of 32-bit words, up to more
than 8192 colours, records in file order and shuffled), on round trips with `colorid merge`, through the ABI call itself, and on one
full-size case at the metric's shape compared in row chunks."""
import os
import struct
import subprocess

import numpy as np
import pytest

import colorid_amd
from colorid_amd import CidError
from test_gpu_merge import compose, header_bytes, random_names, records_of, shuffle_records, write_bxi
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


def write_list(path, names):
    with open(path, "w") as f:
        f.write("".join(n + "\n" for n in names))
    return str(path)


# ---------------------------------------------------------------------------------------------- real genomes (test.sh's parameters)

PHAGE_SETS = {"ab": [B021, B056], "cd": [B051, B545], "one": [B051], "all": [B021, B051, B056, B545]}


@pytest.fixture(scope="module")
def phage_builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("subset_phages")
    for name, accs in PHAGE_SETS.items():
        tsv = d / f"{name}.tsv"
        tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in accs))
        run("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / name), "-r", str(tsv))
        run("build", "-s", "750000", "-n", "4", "-k", "27", "-b", str(d / f"{name}_m"), "-r", str(tsv), "-m", "-v", "15")
    return d


# (flag, the list = a reference list as given to `build -r`, the build the output must equal)
PHAGE_CASES = [("-a", "ab", "ab"), ("-x", "ab", "cd"), ("-a", "one", "one"), ("-a", "all", "all"), ("-x", "cd", "ab")]


@pytest.mark.parametrize("flag,lst,want", PHAGE_CASES)
def test_subset_of_a_build_is_the_build_over_the_kept_lines(phage_builds, flag, lst, want):
    d = phage_builds
    out, err = run("subset", "-b", str(d / "got"), "-i", str(d / "all.bxi"), flag, str(d / f"{lst}.tsv"))
    assert read(d / "got.bxi") == read(d / f"{want}.bxi")
    assert out.splitlines() == [f" Input index : {d / 'all.bxi'}", f" Bigsi file : {d / 'got.bxi'}", "K-mer size: 27",
                                "Bloom filter parameters: num hashes 4, filter size 750000",
                                f"Accessions: {len(PHAGE_SETS[want])} of 4 kept", "Saving BIGSI to file."]
    assert f"Extracting {len(PHAGE_SETS[want])} of 4 accessions from {d / 'all.bxi'}" in err


@pytest.mark.parametrize("flag,lst,want", PHAGE_CASES)
def test_subset_of_a_minimizer_build(phage_builds, flag, lst, want):
    d = phage_builds
    out, _ = run("subset", "-b", str(d / "got_m"), "-i", str(d / "all_m.mxi"), flag, str(d / f"{lst}.tsv"))
    assert read(d / "got_m.mxi") == read(d / f"{want}_m.mxi")
    assert out.splitlines() == [f" Input index : {d / 'all_m.mxi'}", f" Bigsi file : {d / 'got_m.mxi'}", "K-mer size: 27",
                                "Bloom filter parameters: num hashes 4, filter size 750000", "Build with minimizers, minimizer size: 15",
                                f"Accessions: {len(PHAGE_SETS[want])} of 4 kept", "Saving BIGSI to file."]


# ---------------------------------------------------------------------------------------------- synthetic, composed by the oracle

def compose_subset(orc, rng, tmp_path, keep, m=600, m_size=0, shuffle=False, density=0.3, zero_row_frac=0.3):
    """an oracle-written input of len(keep) colours and the expected subset: the kept columns re-packed, saved by the oracle"""
    keep = np.asarray(keep, bool)
    nc, kept = len(keep), np.flatnonzero(keep)
    suffix = ".mxi" if m_size else ".bxi"
    src = random_index(orc, rng, m, 3, 21, nc, density=density, zero_row_frac=zero_row_frac)
    names = random_names(rng, nc)
    n_ref = rng.integers(0, 10**9, size=nc)
    for c in range(nc):
        src.set_color(c, names[c], int(n_ref[c]))
    if m_size:
        src.set_minimizer(m_size)
    bits = np.unpackbits(src.rows().view(np.uint8), axis=1, bitorder="little")[:, :nc].astype(bool)
    exp = orc.Index(m, 3, 21, len(kept))
    if m_size:
        exp.set_minimizer(m_size)
    packed = np.zeros((m, exp.w32 * 32), bool)
    packed[:, :len(kept)] = bits[:, kept]
    exp.rows()[:] = np.packbits(packed, axis=1, bitorder="little").view(np.uint32)
    for j, c in enumerate(kept):
        exp.set_color(j, names[c], int(n_ref[c]))
    src_path, want = str(tmp_path / f"in{suffix}"), str(tmp_path / f"want{suffix}")
    src.save(src_path)
    exp.save(want)
    if shuffle:
        shuffle_records(src_path, rng)
    return src_path, want, [names[c] for c in kept], [names[c] for c in np.flatnonzero(~keep)]


def span(nc, lo, hi):
    k = np.zeros(nc, bool)
    k[lo:hi] = True
    return k


PATTERNS = {
    "dense": lambda nc: np.random.default_rng(nc).random(nc) < 0.8,
    "every_second": lambda nc: np.arange(nc) % 2 == 1,
    "one_in_100": lambda nc: np.arange(nc) % 100 == 37 % nc,
    "single_first": lambda nc: span(nc, 0, 1),
    "single_last": lambda nc: span(nc, nc - 1, nc),
    "all": lambda nc: span(nc, 0, nc),
    "all_but_one": lambda nc: ~span(nc, nc // 2, nc // 2 + 1),
    "prefix_32": lambda nc: span(nc, 0, 32),          # ends exactly on a word border
    "prefix_33": lambda nc: span(nc, 0, 33),          # ... and one past it
    "suffix_from_32": lambda nc: span(nc, 32, nc),    # starts exactly on a word border
    "suffix_from_33": lambda nc: span(nc, 33, nc),
    "suffix_of_32": lambda nc: span(nc, nc - 32, nc),  # 32 kept colours: the output ends exactly on a word border
    "suffix_of_33": lambda nc: span(nc, nc - 33, nc),
}
WIDTHS = (1, 31, 32, 33, 257, 1000, 8300)


def pattern_cases():
    """every (width, pattern) whose pattern fits the width and keeps something (an empty subset is refused); a pattern equal to an
    earlier one of the width is left out"""
    cases = []
    for nc in WIDTHS:
        seen = []
        for name, fn in PATTERNS.items():
            need = {"all_but_one": 2, "prefix_32": 32, "prefix_33": 33, "suffix_from_32": 33, "suffix_from_33": 34, "suffix_of_32": 32,
                    "suffix_of_33": 33}.get(name, 1)
            if nc < need:
                continue
            k = fn(nc)
            assert len(k) == nc
            if not k.any() or any(np.array_equal(k, s) for s in seen):
                continue
            seen.append(k)
            cases.append((nc, name))
    return cases


@pytest.mark.parametrize("nc,pattern", pattern_cases())
@pytest.mark.parametrize("shuffle", [False, True])
def test_subset_matches_oracle_composed_index(orc, tmp_path, nc, pattern, shuffle):
    keep = PATTERNS[pattern](nc)
    rng = np.random.default_rng(nc * 7 + shuffle)
    src, want, kept_names, dropped_names = compose_subset(orc, rng, tmp_path, keep, m=300 if nc > 8192 else 600, shuffle=shuffle)
    # the shorter list says the same: -a with the kept names, or -x with the dropped ones
    if dropped_names and len(dropped_names) < len(kept_names):
        run("subset", "-b", str(tmp_path / "got"), "-i", src, "-x", write_list(tmp_path / "drop.txt", dropped_names))
    else:
        run("subset", "-b", str(tmp_path / "got"), "-i", src, "-a", write_list(tmp_path / "keep.txt", kept_names))
    assert read(tmp_path / "got.bxi") == read(want)


@pytest.mark.parametrize("shuffle", [False, True])
def test_rows_that_become_all_zero_vanish(orc, tmp_path, shuffle):
    """sparse columns kept out of a sparse index: most of the input's rows hold no kept bit and must not be written"""
    rng = np.random.default_rng(11 + shuffle)
    keep = np.arange(300) % 100 == 5
    src, want, kept_names, _ = compose_subset(orc, rng, tmp_path, keep, m=3000, shuffle=shuffle, density=0.02, zero_row_frac=0.3)
    run("subset", "-b", str(tmp_path / "got"), "-i", src, "-a", write_list(tmp_path / "keep.txt", kept_names))
    assert read(tmp_path / "got.bxi") == read(want)
    n_in, n_out = header_bytes(src)[1], header_bytes(str(tmp_path / "got.bxi"))[1]
    assert 0 < n_out < n_in // 4, (n_in, n_out)


def test_subset_matches_oracle_composed_minimizer_index(orc, tmp_path):
    rng = np.random.default_rng(7)
    keep = rng.random(65) < 0.5
    src, want, kept_names, dropped_names = compose_subset(orc, rng, tmp_path, keep, m_size=11, shuffle=True)
    run("subset", "-b", str(tmp_path / "got"), "-i", src, "-x", write_list(tmp_path / "drop.txt", dropped_names))
    assert read(tmp_path / "got.mxi") == read(want)


def test_list_lines_repeat_and_carry_other_columns(orc, tmp_path):
    """only the text before the first TAB counts, empty lines are skipped, a repeated name is the same as naming it once"""
    rng = np.random.default_rng(3)
    keep = np.arange(40) % 3 == 0
    src, want, kept_names, _ = compose_subset(orc, rng, tmp_path, keep)
    lst = tmp_path / "refs.tsv"
    lst.write_text("".join(f"{n}\t/data/{n}.fasta\n\n" for n in reversed(kept_names)) + f"{kept_names[0]}\t/data/a_1.fq.gz\t/data/a_2.fq.gz\r\n")
    run("subset", "-b", str(tmp_path / "got"), "-i", src, "-a", str(lst))
    assert read(tmp_path / "got.bxi") == read(want)


# ---------------------------------------------------------------------------------------------- round trips with merge

def names_of(path):
    raw = read(path)
    at = 32 if path.endswith(".mxi") else 24
    nc = struct.unpack_from("<Q", raw, at)[0]
    at += 8
    names = []
    for _ in range(nc):
        n = struct.unpack_from("<Q", raw, at + 8)[0]
        names.append(raw[at + 16:at + 16 + n].decode())
        at += 16 + n
    return names


@pytest.mark.parametrize("split", [(31, 33), (100, 157), (1, 64)])
def test_subset_of_a_merge_gives_the_input_back(orc, tmp_path, split):
    """subset(merge(a, b), names(a)) == a, and the same for b by exclusion: replace one accession = drop it, build the new one, merge"""
    rng = np.random.default_rng(sum(split))
    (a, b), _ = compose(orc, rng, tmp_path, split)
    run("merge", "-b", str(tmp_path / "ab"), "-i", a, b)
    names_a = write_list(tmp_path / "a.txt", names_of(a))
    run("subset", "-b", str(tmp_path / "a_again"), "-i", str(tmp_path / "ab.bxi"), "-a", names_a)
    assert read(tmp_path / "a_again.bxi") == read(a)
    run("subset", "-b", str(tmp_path / "b_again"), "-i", str(tmp_path / "ab.bxi"), "-x", names_a)
    assert read(tmp_path / "b_again.bxi") == read(b)


@pytest.mark.parametrize("nc,shuffle", [(64, False), (257, True), (1000, True)])
def test_merge_of_a_subset_and_its_complement_gives_the_index_back(orc, tmp_path, nc, shuffle):
    rng = np.random.default_rng(nc)
    keep = rng.random(nc) < 0.5                       # an interleaved random split
    src, _, kept_names, _ = compose_subset(orc, rng, tmp_path, keep)
    whole = read(src)                                 # as the oracle saved it: rows ascending
    if shuffle:
        shuffle_records(src, rng)
    lst = write_list(tmp_path / "s.txt", kept_names)
    run("subset", "-b", str(tmp_path / "s"), "-i", src, "-a", lst)
    run("subset", "-b", str(tmp_path / "t"), "-i", src, "-x", lst)
    run("merge", "-b", str(tmp_path / "back"), "-i", str(tmp_path / "t.bxi"), str(tmp_path / "s.bxi"))
    assert read(tmp_path / "back.bxi") == whole


# ---------------------------------------------------------------------------------------------- the ABI call

def test_put_records_subset_extracts_what_numpy_says(hip_ctx):
    rng = np.random.default_rng(5)
    nc_file, m = 150, 64
    keep = rng.random(nc_file) < 0.3
    keep[[0, 31, 32, 63, 64, 149]] = True
    k = int(keep.sum())
    assert k % 32                                      # the last output word has unused high bits
    bits = rng.random((m, nc_file)) < 0.5
    bits[:, ~keep] = True                              # everything that is dropped is set: nothing of it may leak into the output
    packed = np.zeros((m, 5 * 32), bool)
    packed[:, :nc_file] = bits
    words = np.packbits(packed, axis=1, bitorder="little").view(np.uint32)
    put = [r for r in range(m) if r % 5]               # rows never put stay zero
    ix = colorid_amd.Index(hip_ctx, m, 2, 21, k)
    half = len(put) // 2
    ix.put_records_subset(records_of({r: words[r] for r in put[:half]}, nc_file), nc_file, keep)       # two chunks of one file
    ix.put_records_subset(records_of({r: words[r] for r in put[half:]}, nc_file), nc_file, keep)
    ix.finalize()
    got = ix.get_rows(list(range(m)))
    want_bits = np.zeros((m, ix.w32 * 32), bool)
    want_bits[:, :k] = bits[:, keep]
    want_bits[[r for r in range(m) if r % 5 == 0]] = False
    want = np.packbits(want_bits, axis=1, bitorder="little").view(np.uint32)
    assert np.array_equal(got, want)
    assert not (got[:, -1] >> np.uint32(k % 32)).any()  # bits at and beyond n_colors are zero
    ix.close()


def test_put_records_subset_stores_rows(hip_ctx):
    """rows are stored, not OR-ed: a row put again is replaced"""
    ix = colorid_amd.Index(hip_ctx, 10, 2, 21, 2)
    keep = np.array([False, True, False, True])
    ix.put_records_subset(records_of({3: [0b1010]}, 4), 4, keep)
    ix.put_records_subset(records_of({3: [0b0010], 4: [0b1000]}, 4), 4, keep)
    ix.finalize()
    assert ix.get_rows([3, 4, 5]).tolist() == [[0b01], [0b10], [0]]
    ix.close()


def test_put_records_subset_refusals(hip_ctx):
    ix = colorid_amd.Index(hip_ctx, 100, 2, 21, 2)
    rec = records_of({5: [0b101]}, 3)
    good = np.array([True, False, True])
    for bad in ([True, False, False], [True, True, True]):                       # popcount != the index's n_colors
        with pytest.raises(CidError) as e:
            ix.put_records_subset(rec, 3, np.array(bad))
        assert e.value.code == -1
    with pytest.raises(CidError) as e:                                           # a stray bit at the file's n_colors
        ix.put_records_subset(rec, 3, np.array([0b1001], np.uint32))
    assert e.value.code == -1
    with pytest.raises(CidError) as e:                                           # a file of no colours
        ix.put_records_subset(b"", 0, np.array([0b11], np.uint32))
    assert e.value.code == -1
    # malformed records, with cid_index_put_records' text
    with pytest.raises(CidError) as e:                                           # two words announced, the file's shape has one
        ix.put_records_subset(struct.pack("<QQIQ", 5, 2, 0b101, 3), 3, good)
    assert e.value.code == -1 and "word count != ceil(n_colors/32)" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit count that is not the file's
        ix.put_records_subset(records_of({5: [0b101]}, 4), 3, good)
    assert e.value.code == -1 and "bit count != n_colors" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a row past bloom_size
        ix.put_records_subset(records_of({100: [0b101]}, 3), 3, good)
    assert e.value.code == -1 and "row >= bloom_size" in str(e.value)
    with pytest.raises(CidError) as e:                                           # a bit past the file's 3 colours
        ix.put_records_subset(records_of({5: [0b1101]}, 3), 3, good)
    assert e.value.code == -1 and "bits beyond n_colors" in str(e.value)
    ix.put_records_subset(rec, 3, good)
    ix.finalize()
    assert ix.get_rows([5, 100 - 1]).tolist() == [[0b11], [0]]
    with pytest.raises(CidError) as e:
        ix.put_records_subset(rec, 3, good)
    assert e.value.code == -5
    ix.close()


# ---------------------------------------------------------------------------------------------- full size

def check_subset(path, m, rows, kept, names):
    """the subset file against the numpy extraction of the input's rows, in row chunks (never a dense bool array of the whole index)"""
    start, n_rows, rec = header_bytes(path)
    w_out = (len(kept) + 31) // 32
    assert rec == 24 + 4 * w_out
    recs = np.memmap(path, dtype=np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (w_out,)), ("nb", "<u8")]), mode="r", offset=start,
                     shape=(n_rows,))
    seen = 0
    step = 1 << 21
    for r0 in range(0, m, step):
        bits = np.unpackbits(rows[r0:r0 + step].view(np.uint8), axis=1, bitorder="little")[:, kept]
        want_w = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint32)
        nz = np.flatnonzero(want_w.any(axis=1))
        got = recs[seen:seen + len(nz)]
        assert np.array_equal(got["row"], nz + r0), r0
        assert np.array_equal(got["w"], want_w[nz]), r0
        assert (got["nw"] == w_out).all() and (got["nb"] == len(kept)).all()
        seen += len(nz)
    assert seen == n_rows
    del recs
    assert names_of(path) == [names[c] for c in kept]
    with open(path, "rb") as f:
        f.seek(start + n_rows * rec)
        tail = f.read()
    assert tail == struct.pack("<Q", len(kept)) + b"".join(struct.pack("<Q", len(names[c])) + names[c].encode() + struct.pack("<Q", 1000 + c)
                                                           for c in kept)


def full_size_input(d, rng, m=50_000_000, nc=256, n_keep=128):
    """a 256-colour input of the metric's shape (m = 50 M, n = 4, k = 31; random rows, a fifth of them zero) and 128 colours to keep,
    chosen by a seeded permutation; returns the path, the rows, the names and the kept colours (ascending)"""
    names = random_names(rng, nc)
    rows = rng.integers(0, 2**32, size=(m, nc // 32), dtype=np.uint32) & rng.integers(0, 2**32, size=(m, nc // 32), dtype=np.uint32)
    rows[rng.random(m) < 0.2] = 0
    src = str(d / "in.bxi")
    write_bxi(src, m, 4, 31, names, rows)
    kept = np.sort(rng.permutation(nc)[:n_keep])
    return src, rows, names, kept


@pytest.mark.timeout(1800)
def test_full_size_subset(tmp_path):
    """the metric's shape (m = 50 M, n = 4, k = 31): 128 colours, chosen by a seeded permutation, out of a 256-colour input"""
    import torch
    m = 50_000_000
    need = 4 << 30       # the 128-colour output index (0.8 GB), one 256 MiB upload chunk, the records read back: well under 4 GiB
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        print(f"test_full_size_subset: skipped, the device has {free >> 20} MiB free, the case needs {need >> 20} MiB")
        pytest.skip(f"device memory: {free >> 20} MiB free, {need >> 20} MiB needed")
    src, rows, names, kept = full_size_input(tmp_path, np.random.default_rng(41), m)
    out, _ = run("subset", "-b", str(tmp_path / "sub"), "-i", src, "-a", write_list(tmp_path / "keep.txt", [names[c] for c in kept]))
    assert "Accessions: 128 of 256 kept" in out
    check_subset(str(tmp_path / "sub.bxi"), m, rows, kept, names)
