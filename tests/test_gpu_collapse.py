"""`colorid collapse` and cid_index_put_records_grouped on the GPU.  The contract: the row records of a collapsed index are the ones `build`
writes over a reference list with one line per group whose FASTA is the members' FASTA files joined — checked on the four phages of
test.sh; on synthetic indices whose expected file the oracle saves from the OR of the members' columns (maps from identity to all into
one, borders of 32-bit words, up to more than 8192 colours, records in file order and shuffled, .bxi and .mxi); on renames and
reorderings; through the ABI call itself with its counters; and on round trips with `subset` and `merge`.  n_ref_kmers of a group of
several is an estimate: checked against a restatement of the rule, and on real genomes against `build`'s exact count."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest

import colorid_amd
from colorid_amd import CidError
from test_gpu_merge import compose, header_bytes, random_names, shuffle_records
from test_gpu_subset import names_of, read, run, write_list

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REFS = os.path.join(HERE, "golden", "refs")
B021, B051, B056, B545 = (f"Listeria_phage_{n}" for n in ("B021", "B051", "B056", "B545"))
REPORT_HEADER = "group\tmembers\tn_ref_kmers\tn_ref_sum\tbits\tfill\tfp_stated\tfp_measured"


def py_n_ref(m, n, n_i, bits_i, bits_group):
    """the rule of `collapse` for a group's n_ref_kmers, restated"""
    if len(n_i) == 1:
        return n_i[0]
    if any(v == 0 for v in n_i):
        return 0
    if bits_group >= m or any(b >= m for b in bits_i):
        return sum(n_i)
    est = lambda x: -(m / n) * math.log1p(-x / m)                      # noqa: E731
    members = sum(est(b) for b in bits_i)
    if not members > 0:
        return sum(n_i)
    return min(max(math.floor(sum(n_i) * est(bits_group) / members + 0.5), max(n_i)), sum(n_i))


def write_groups(path, pairs):
    with open(path, "w") as f:
        f.write("".join(f"{a}\t{g}\n" for a, g in pairs))
    return str(path)


def record_bytes_of(path):
    """a file up to its row records (header and colours), and the records"""
    start, n_rows, rec = header_bytes(path)
    raw = read(path)
    return raw[:start], raw[start:start + n_rows * rec]


def tail_of(path):
    """[(name, n_ref_kmers)] as the file's tail states them"""
    start, n_rows, rec = header_bytes(path)
    raw = read(path)
    at = start + n_rows * rec
    n = struct.unpack_from("<Q", raw, at)[0]
    at += 8
    out = []
    for _ in range(n):
        ln = struct.unpack_from("<Q", raw, at)[0]
        out.append((raw[at + 8:at + 8 + ln].decode(), struct.unpack_from("<Q", raw, at + 8 + ln)[0]))
        at += 16 + ln
    assert at == len(raw)
    return out


def report_of(path):
    lines = open(path).read().splitlines()
    assert lines[0] == REPORT_HEADER
    return [ln.split("\t") for ln in lines[1:]]


def column_sums(rows, nc):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :nc].sum(axis=0, dtype=np.uint64)


def collapse(out_stem, src, groups):
    return run("collapse", "-b", str(out_stem), "-i", src, "-g", groups)


# ---------------------------------------------------------------------------------------------- real genomes (test.sh's parameters)

PHAGE_GROUPS = {"pairs": {"Listeria_phage_A": [B021, B056], "Listeria_phage_B": [B051, B545]},
                "one": {"Listeria_phages": [B021, B051, B056, B545]}}
M, N_HASH, K = 750000, 4, 27


@pytest.fixture(scope="module")
def phage_builds(tmp_path_factory):
    """the strain-level builds (.bxi, .mxi) and, per grouping, the build over one line per group: the members' files concatenated"""
    d = tmp_path_factory.mktemp("collapse_phages")

    def build(stem, tsv):
        run("build", "-s", str(M), "-n", str(N_HASH), "-k", str(K), "-b", str(d / stem), "-r", str(tsv))
        run("build", "-s", str(M), "-n", str(N_HASH), "-k", str(K), "-b", str(d / f"{stem}_m"), "-r", str(tsv), "-m", "-v", "15")

    tsv = d / "all.tsv"
    tsv.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in (B021, B051, B056, B545)))
    build("all", tsv)
    for name, groups in PHAGE_GROUPS.items():
        lines = []
        for g, members in groups.items():
            with open(d / f"{g}.fasta", "wb") as f:
                for mname in members:
                    text = read(os.path.join(REFS, mname + ".fasta"))
                    f.write(text if text.endswith(b"\n") else text + b"\n")
            lines.append(f"{g}\t{d / (g + '.fasta')}\n")
        (d / f"{name}.tsv").write_text("".join(lines))
        (d / f"{name}_groups.tsv").write_text("".join(f"{mname}\t{g}\n" for g, members in groups.items() for mname in members))
        build(name, d / f"{name}.tsv")
    return d


def check_phages(orc, d, grouping, suffix, stem_tail):
    groups = PHAGE_GROUPS[grouping]
    src, want, got = str(d / f"all{stem_tail}{suffix}"), str(d / f"{grouping}{stem_tail}{suffix}"), str(d / f"got_{grouping}{stem_tail}{suffix}")
    out, err = collapse(got[:-4], src, str(d / f"{grouping}_groups.tsv"))
    lines = [f" Input index : {src}", f" Bigsi file : {got}", f"K-mer size: {K}", f"Bloom filter parameters: num hashes {N_HASH}, filter size {M}"]
    if suffix == ".mxi":
        lines.append("Build with minimizers, minimizer size: 15")
    assert out.splitlines() == lines + [f"Accessions: 4 in {len(groups)} groups", "Saving BIGSI to file."]
    assert f"Collapsing 4 accessions of {src} into {len(groups)} groups" in err
    # header, colours and every row record, byte for byte; and once more as the oracle reads them
    assert record_bytes_of(got) == record_bytes_of(want)
    g_ix, w_ix, s_ix = orc.Index.read(got), orc.Index.read(want), orc.Index.read(src)
    assert g_ix.colors() == w_ix.colors() == sorted(groups) and np.array_equal(g_ix.rows(), w_ix.rows())
    assert (g_ix.m, g_ix.n_hash, g_ix.k, g_ix.m_size) == (w_ix.m, w_ix.n_hash, w_ix.k, w_ix.m_size)
    # the report: one line per group; bits are the output's column sums
    bits_out, bits_in = column_sums(g_ix.rows(), len(groups)), column_sums(s_ix.rows(), 4)
    n_in = dict(zip(s_ix.colors(), s_ix.n_ref_kmers()))
    x_in = dict(zip(s_ix.colors(), (int(b) for b in bits_in)))
    rep = report_of(got[:-4] + "_groups.tsv")
    assert [r[0] for r in rep] == sorted(groups)
    for j, (g, r) in enumerate(zip(sorted(groups), rep)):
        n_i = [n_in[a] for a in groups[g]]
        written, exact = g_ix.n_ref_kmers()[j], w_ix.n_ref_kmers()[j]
        fill = int(bits_out[j]) / M
        assert r[1] == ",".join(groups[g]) and int(r[2]) == written and int(r[3]) == sum(n_i) and int(r[4]) == int(bits_out[j])
        assert all(re.fullmatch(r"\d+\.\d{6}", v) for v in r[5:8]), r     # %.6f, as cmp_accessions.tsv
        for v, want_v in zip(r[5:8], (fill, orc.false_prob(M, N_HASH, written), fill ** N_HASH)):
            assert abs(float(v) - want_v) <= 1e-6, (r, want_v)
        print(f"{grouping}{suffix} {g}: n_ref_kmers written {written}, build counts {exact}, members {n_i}, bits {int(bits_out[j])}")
        assert max(n_i) <= written <= sum(n_i)
        assert abs(written - py_n_ref(M, N_HASH, n_i, [x_in[a] for a in groups[g]], int(bits_out[j]))) <= 1
        if suffix == ".bxi":   # the estimate against build's exact count of the union, within six standard errors of the fill estimator
            t = N_HASH * exact / M
            se = math.sqrt(M * (math.exp(t) - 1 - t)) / N_HASH
            print(f"    error {written - exact:+d}, se {se:.1f}")
            assert abs(written - exact) <= 6 * se + 1
    return got, want


@pytest.mark.parametrize("grouping", ["pairs", "one"])
def test_collapse_of_a_build_is_the_build_over_the_joined_genomes(orc, phage_builds, grouping):
    d = phage_builds
    got, want = check_phages(orc, d, grouping, ".bxi", "")
    query = os.path.join(REFS, B021 + ".fasta")
    assert run("search", "-b", got, "-q", query, "-g")[0] == run("search", "-b", want, "-q", query, "-g")[0]


@pytest.mark.parametrize("grouping", ["pairs", "one"])
def test_collapse_of_a_minimizer_build(orc, phage_builds, grouping):
    check_phages(orc, phage_builds, grouping, ".mxi", "_m")


# ---------------------------------------------------------------------------------------------- synthetic, composed by the oracle

def compose_collapse(orc, rng, tmp_path, labels, m=600, m_size=0, shuffle=False, unlisted=(), n_ref=None, full_columns=(), density=0.3,
                     zero_row_frac=0.3):
    """an oracle-written input of len(labels) colours, a groups file that puts colour c into group labels[c] (the groups named at random;
    a label in `unlisted` must be a singleton: its accession is left out of the file and keeps its name), and the expected output saved
    by the oracle: colours in byte order of the names, every column the OR of its members', n_ref_kmers by the restated rule.
    Returns (input path, expected path, groups path, [(name, member colours)] in output order)."""
    labels = np.asarray(labels)
    nc, n_groups = len(labels), int(labels.max()) + 1
    suffix = ".mxi" if m_size else ".bxi"
    bits = rng.random((m, nc)) < density
    bits[rng.random(m) < zero_row_frac] = False
    for c in full_columns:
        bits[:, c] = True
    names = random_names(rng, nc)                                     # the alphabet has no 'x': no group is called as an accession
    gnames = ["x" + s for s in random_names(rng, n_groups)]
    n_ref = rng.integers(1, 10**9, size=nc) if n_ref is None else np.asarray(n_ref)

    def save(path, cols_bits, colours):
        ix = orc.Index(m, 3, 21, cols_bits.shape[1])
        if m_size:
            ix.set_minimizer(m_size)
        packed = np.zeros((m, ix.w32 * 32), bool)
        packed[:, :cols_bits.shape[1]] = cols_bits
        ix.rows()[:] = np.packbits(packed, axis=1, bitorder="little").view(np.uint32)
        for j, (name, n) in enumerate(colours):
            ix.set_color(j, name, int(n))
        ix.save(path)

    src, want, groups_path = str(tmp_path / f"in{suffix}"), str(tmp_path / f"want{suffix}"), str(tmp_path / "groups.tsv")
    save(src, bits, list(zip(names, n_ref)))
    members = [np.flatnonzero(labels == g) for g in range(n_groups)]
    assert all(len(mb) for mb in members) and all(len(members[g]) == 1 for g in unlisted)
    named = sorted(((names[members[g][0]] if g in unlisted else gnames[g], members[g]) for g in range(n_groups)), key=lambda t: t[0].encode())
    write_groups(groups_path, [(names[c], gnames[labels[c]]) for c in rng.permutation(nc) if labels[c] not in unlisted])
    x_in = bits.sum(axis=0)
    out_bits = np.stack([bits[:, mb].any(axis=1) for _, mb in named], axis=1)
    x_out = out_bits.sum(axis=0)
    exp_n = [py_n_ref(m, 3, [int(n_ref[c]) for c in mb], [int(x_in[c]) for c in mb], int(x_out[j])) for j, (_, mb) in enumerate(named)]
    save(want, out_bits, [(name, exp_n[j]) for j, (name, _) in enumerate(named)])
    if shuffle:
        shuffle_records(src, rng)
    return src, want, groups_path, named


def border_labels(nc):
    """groups across the borders of file words: {31, 32} and, where they exist, {63, 64, 65}; the rest singletons"""
    label = np.arange(nc)
    label[32] = 31
    label[64:66] = 63
    return np.unique(label, return_inverse=True)[1]


def all_but_three(nc):
    lab = np.full(nc, 3)
    lab[0], lab[nc // 2], lab[nc - 1] = 0, 1, 2
    return lab


MAPS = {
    "identity": (1, lambda nc: np.arange(nc)),
    "reverse": (2, lambda nc: nc - 1 - np.arange(nc)),
    "all_into_one": (1, lambda nc: np.zeros(nc, int)),
    "neighbour_pairs": (2, lambda nc: np.arange(nc) // 2),
    "mod_2": (2, lambda nc: np.arange(nc) % 2),
    "mod_33": (33, lambda nc: np.arange(nc) % 33),
    "borders": (33, border_labels),
    "all_but_three": (4, all_but_three),
    "random_1": (1, lambda nc: np.zeros(nc, int)),
    "random_2": (2, lambda nc: random_onto(nc, 2)),
    "random_33": (33, lambda nc: random_onto(nc, 33)),
    "random_n": (2, lambda nc: random_onto(nc, nc)),
}
WIDTHS = (1, 31, 32, 33, 64, 65, 300)


def random_onto(nc, g):
    """a seeded random assignment of nc colours onto all of g groups"""
    rng = np.random.default_rng(1000 * nc + g)
    return rng.permutation(np.concatenate([np.arange(g), rng.integers(0, g, size=nc - g)]))


def map_cases():
    """every (width, map) the width is wide enough for; a map equal to an earlier one of the width is left out; 8200 colours (records too
    wide for the kernel's LDS tile) with three maps only"""
    cases = []
    for nc in WIDTHS:
        seen = []
        for name, (need, fn) in MAPS.items():
            if nc < need:
                continue
            lab = fn(nc)
            assert len(lab) == nc and set(lab) == set(range(int(lab.max()) + 1))
            if any(np.array_equal(lab, s) for s in seen):
                continue
            seen.append(lab)
            cases.append((nc, name))
    return cases + [(8200, "mod_33"), (8200, "neighbour_pairs"), (8200, "all_into_one")]


def check_collapsed(got, want, named):
    """header, colours and rows exactly; n_ref_kmers within 1 of the restated rule, and exactly where the rule does no arithmetic"""
    assert record_bytes_of(got) == record_bytes_of(want)
    got_tail, want_tail = tail_of(got), tail_of(want)
    assert [t[0] for t in got_tail] == [t[0] for t in want_tail] == [name for name, _ in named]
    for (name, g), (_, w) in zip(got_tail, want_tail):
        assert abs(g - w) <= 1, (name, g, w)


@pytest.mark.parametrize("nc,which", map_cases())
@pytest.mark.parametrize("shuffle", [False, True])
def test_collapse_matches_oracle_composed_index(orc, tmp_path, nc, which, shuffle):
    rng = np.random.default_rng(nc * 7 + shuffle)
    m_size = 11 if (nc + len(which) + shuffle) % 2 else 0             # .bxi and .mxi alternate over the cases
    src, want, groups, named = compose_collapse(orc, rng, tmp_path, MAPS[which][1](nc), m=300 if nc > 8192 else 600, m_size=m_size, shuffle=shuffle)
    out, _ = collapse(tmp_path / "got", src, groups)
    assert f"Accessions: {nc} in {len(named)} groups" in out
    suffix = ".mxi" if m_size else ".bxi"
    check_collapsed(str(tmp_path / f"got{suffix}"), want, named)
    rep = report_of(tmp_path / "got_groups.tsv")
    assert [r[0] for r in rep] == [name for name, _ in named]
    w_ix = orc.Index.read(want)                                        # (rows() is a view of the oracle's memory: the index must outlive it)
    assert [int(r[4]) for r in rep] == [int(b) for b in column_sums(w_ix.rows(), len(named))]


@pytest.mark.parametrize("m_size", [0, 11])
def test_counts_of_zero_and_full_columns_are_exact(orc, tmp_path, m_size):
    """a member without a count (build -m from reads records none) -> 0; a full column among the members -> the sum of the counts; a
    singleton -> its own count: no arithmetic, so no tolerance"""
    rng = np.random.default_rng(5 + m_size)
    labels = np.array([0, 0, 1, 1, 1, 2, 3, 3])                       # group 0 has a zero count, group 1 a full column, 2 is a singleton
    n_ref = [700, 0, 10, 20, 30, 12345, 400, 500]
    src, want, groups, named = compose_collapse(orc, rng, tmp_path, labels, m_size=m_size, n_ref=n_ref, full_columns=(3,), shuffle=True)
    collapse(tmp_path / "got", src, groups)
    suffix = ".mxi" if m_size else ".bxi"
    check_collapsed(str(tmp_path / f"got{suffix}"), want, named)
    by_members = {tuple(int(c) for c in mb): n for (_, mb), (_, n) in zip(named, tail_of(str(tmp_path / f"got{suffix}")))}
    assert by_members[(0, 1)] == 0 and by_members[(2, 3, 4)] == 60 and by_members[(5,)] == 12345 and 500 <= by_members[(6, 7)] <= 900


# ---------------------------------------------------------------------------------------------- rename and reorder

@pytest.mark.parametrize("nc,m_size", [(5, 0), (40, 0), (70, 11)])
def test_rename_and_reorder(orc, tmp_path, nc, m_size):
    """every accession its own group under a new random name: the columns permuted into the new names' order, n_ref_kmers included"""
    rng = np.random.default_rng(nc)
    src, want, groups, named = compose_collapse(orc, rng, tmp_path, rng.permutation(nc), m_size=m_size)
    assert [int(mb[0]) for _, mb in named] != list(range(nc))          # the new names do reorder
    collapse(tmp_path / "got", src, groups)
    suffix = ".mxi" if m_size else ".bxi"
    assert read(tmp_path / f"got{suffix}") == read(want)


def test_unlisted_accessions_stay_and_empty_file_gives_the_input_back(orc, tmp_path):
    rng = np.random.default_rng(9)
    labels = np.array([0, 1, 1, 2, 3, 3, 3, 4])                       # 0, 2 and 4 are singletons that the file does not list
    src, want, groups, named = compose_collapse(orc, rng, tmp_path, labels, unlisted=(0, 2, 4))
    collapse(tmp_path / "got", src, groups)
    check_collapsed(str(tmp_path / "got.bxi"), want, named)
    for text in ("", "\n\r\n"):
        (tmp_path / "empty.tsv").write_text(text)
        out, _ = collapse(tmp_path / "same", src, str(tmp_path / "empty.tsv"))
        assert "Accessions: 8 in 8 groups" in out
        assert read(tmp_path / "same.bxi") == read(src)


def test_groups_file_carries_other_columns(orc, tmp_path):
    """what follows a second TAB is ignored, empty lines are skipped"""
    rng = np.random.default_rng(3)
    src, want, groups, named = compose_collapse(orc, rng, tmp_path, np.arange(40) % 3)
    lines = open(groups).read().splitlines()
    (tmp_path / "wide.tsv").write_text("".join(f"{ln}\tcomment {i}\tmore\r\n\n" for i, ln in enumerate(lines)))
    collapse(tmp_path / "got", src, str(tmp_path / "wide.tsv"))
    check_collapsed(str(tmp_path / "got.bxi"), want, named)


# ---------------------------------------------------------------------------------------------- the ABI call

def dense_records(bits, rows):
    """.bxi records of the given rows of a bool matrix (rows x file colours)"""
    nc = bits.shape[1]
    w32 = (nc + 31) // 32
    packed = np.zeros((len(rows), w32 * 32), bool)
    packed[:, :nc] = bits[rows]
    out = np.empty(len(rows), np.dtype([("row", "<u8"), ("nw", "<u8"), ("w", "<u4", (w32,)), ("nb", "<u8")]))
    out["row"], out["nw"], out["nb"] = rows, w32, nc
    out["w"] = np.packbits(packed, axis=1, bitorder="little").view(np.uint32).reshape(len(rows), w32)
    return out.tobytes()


def grouped_rows(bits, group_of, n_groups):
    out = np.zeros((bits.shape[0], (n_groups + 31) // 32 * 32), bool)
    for g in range(n_groups):
        out[:, g] = bits[:, group_of == g].any(axis=1)
    return out


@pytest.mark.parametrize("n_calls", [1, 2, 7])
@pytest.mark.parametrize("nc_file,n_groups", [(150, 40), (3872, 33), (3873, 33)])   # 3872: the widest records the kernel stages in LDS
def test_put_records_grouped_rows_and_counters(hip_ctx, n_calls, nc_file, n_groups):
    """one file in 1, 2 and 7 calls with a call of no records in between: the rows are numpy's ORs, both counters numpy's column sums"""
    rng = np.random.default_rng(nc_file + n_calls)
    m = 500
    group_of = random_onto(nc_file, n_groups).astype(np.uint32)
    bits = rng.random((m, nc_file)) < 0.2
    put = rng.permutation([r for r in range(m) if r % 5])             # rows never put stay zero; any order
    ix = colorid_amd.Index(hip_ctx, m, 2, 21, n_groups)
    bits_file, bits_index = np.full(nc_file, 7, np.uint64), np.full(n_groups, 9, np.uint64)   # the counters are ADDED to
    for i, part in enumerate(np.array_split(put, n_calls)):
        ix.put_records_grouped(dense_records(bits, part), nc_file, group_of, bits_file, bits_index)
        if i == 0:
            ix.put_records_grouped(b"", nc_file, group_of, bits_file, bits_index)
    ix.finalize()
    want_bits = grouped_rows(bits, group_of, n_groups)
    want_bits[[r for r in range(m) if r % 5 == 0]] = False
    got = ix.get_rows(list(range(m)))
    assert np.array_equal(got, np.packbits(want_bits, axis=1, bitorder="little").view(np.uint32))
    if n_groups % 32:
        assert not (got[:, -1] >> np.uint32(n_groups % 32)).any()      # bits at and beyond n_colors are zero
    assert np.array_equal(bits_file - 7, bits[np.sort(put)].sum(axis=0).astype(np.uint64))
    assert np.array_equal(bits_index - 9, want_bits[:, :n_groups].sum(axis=0).astype(np.uint64))
    ix.close()


def test_put_records_grouped_without_counters_and_disjoint_calls(hip_ctx):
    """bits_file=None and bits_index=None are accepted, each alone too; rows of a second call leave the first call's rows alone"""
    rng = np.random.default_rng(2)
    m, nc_file, n_groups = 200, 70, 3
    group_of = (np.arange(nc_file) % n_groups).astype(np.uint32)
    bits = rng.random((m, nc_file)) < 0.05
    ix = colorid_amd.Index(hip_ctx, m, 2, 21, n_groups)
    first, second, third = np.arange(0, 60), np.arange(60, 130), np.arange(130, 200)
    ix.put_records_grouped(dense_records(bits, first), nc_file, group_of)
    bits_index = np.zeros(n_groups, np.uint64)
    ix.put_records_grouped(dense_records(bits, second), nc_file, group_of, None, bits_index)
    bits_file = np.zeros(nc_file, np.uint64)
    ix.put_records_grouped(dense_records(bits, third), nc_file, group_of, bits_file, None)
    want_bits = grouped_rows(bits, group_of, n_groups)
    assert np.array_equal(ix.get_rows(list(range(m))), np.packbits(want_bits, axis=1, bitorder="little").view(np.uint32))
    assert np.array_equal(bits_index, want_bits[second, :n_groups].sum(axis=0).astype(np.uint64))
    assert np.array_equal(bits_file, bits[third].sum(axis=0).astype(np.uint64))
    ix.finalize()
    ix.close()


def test_put_records_grouped_refusals(hip_ctx):
    m, nc_file, n_groups = 100, 3, 2
    ix = colorid_amd.Index(hip_ctx, m, 2, 21, n_groups)
    good = np.array([0, 1, 0], np.uint32)
    rec = struct.pack("<QQIQ", 5, 1, 0b101, 3)
    for bad in ([0, 0, 0], [1, 1, 1], [0, 2, 1], [0, 1, 2**32 - 1]):   # an index colour without a member (twice), an entry >= n_colors (twice)
        with pytest.raises(CidError) as e:
            ix.put_records_grouped(rec, nc_file, np.array(bad, np.uint32))
        assert e.value.code == -1
    gp = good.ctypes.data_as(ctypes.c_void_p)
    assert ix.lib.cid_index_put_records_grouped(None, None, 0, 3, gp, None, None) == -1     # null arguments, a file of no colours
    assert ix.lib.cid_index_put_records_grouped(ix.h, None, 1, 3, gp, None, None) == -1
    assert ix.lib.cid_index_put_records_grouped(ix.h, None, 0, 3, None, None, None) == -1
    assert ix.lib.cid_index_put_records_grouped(ix.h, None, 0, 0, gp, None, None) == -1
    # a call with one malformed record among good ones: cid_index_put_records' message, and nothing has changed
    ix.put_records_grouped(struct.pack("<QQIQ", 7, 1, 0b011, 3), nc_file, good)
    before = ix.get_rows(list(range(m)))
    assert before[7].tolist() == [0b11]
    for bad_rec, text in ((struct.pack("<QQIQ", 9, 2, 0b101, 3), "word count != ceil(n_colors/32)"),
                          (struct.pack("<QQIQ", m, 1, 0b101, 3), "row >= bloom_size"),
                          (struct.pack("<QQIQ", 9, 1, 0b1101, 3), "bits beyond n_colors")):
        bits_file, bits_index = np.full(nc_file, 3, np.uint64), np.full(n_groups, 4, np.uint64)
        call = rec + bad_rec + struct.pack("<QQIQ", 11, 1, 0b111, 3)
        with pytest.raises(CidError) as e:
            ix.put_records_grouped(call, nc_file, good, bits_file, bits_index)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
        assert np.array_equal(ix.get_rows(list(range(m))), before)
        assert (bits_file == 3).all() and (bits_index == 4).all()
    ix.put_records_grouped(rec, nc_file, good)
    ix.finalize()
    assert ix.get_rows([5, 7, m - 1]).tolist() == [[0b01], [0b11], [0]]
    with pytest.raises(CidError) as e:
        ix.put_records_grouped(rec, nc_file, good)
    assert e.value.code == -5
    ix.close()


# ---------------------------------------------------------------------------------------------- round trips

def rows_and_colours(orc, path):
    ix = orc.Index.read(path)
    return ix.colors(), ix.rows().copy()


def test_collapse_then_subset_is_subset_then_collapse(orc, tmp_path):
    rng = np.random.default_rng(21)
    labels = random_onto(90, 7)
    src, _, groups, named = compose_collapse(orc, rng, tmp_path, labels, shuffle=True)
    name, members = named[3]
    in_names = names_of(src)
    collapse(tmp_path / "c", src, groups)
    run("subset", "-b", str(tmp_path / "cs"), "-i", str(tmp_path / "c.bxi"), "-a", write_list(tmp_path / "g.txt", [name]))
    run("subset", "-b", str(tmp_path / "s"), "-i", src, "-a", write_list(tmp_path / "m.txt", [in_names[c] for c in members]))
    collapse(tmp_path / "sc", str(tmp_path / "s.bxi"), write_groups(tmp_path / "one.tsv", [(in_names[c], name) for c in members]))
    a, b = rows_and_colours(orc, str(tmp_path / "cs.bxi")), rows_and_colours(orc, str(tmp_path / "sc.bxi"))
    assert a[0] == b[0] == [name] and np.array_equal(a[1], b[1]) and a[1].any()


def test_merge_of_collapsed_halves_is_collapse_of_the_merge(orc, tmp_path):
    rng = np.random.default_rng(22)
    (a, b), _ = compose(orc, rng, tmp_path, (45, 70))
    pairs = []
    for tag, path, n_groups in (("xa", a, 6), ("xb", b, 33)):
        names = names_of(path)
        lab = random_onto(len(names), n_groups)
        mine = [(n, f"{tag}{lab[c]:03d}") for c, n in enumerate(names)]
        collapse(tmp_path / f"c_{tag}", path, write_groups(tmp_path / f"{tag}.tsv", mine))
        pairs += mine
    run("merge", "-b", str(tmp_path / "merged_halves"), "-i", str(tmp_path / "c_xa.bxi"), str(tmp_path / "c_xb.bxi"))
    run("merge", "-b", str(tmp_path / "ab"), "-i", a, b)
    collapse(tmp_path / "collapsed_merge", str(tmp_path / "ab.bxi"), write_groups(tmp_path / "all.tsv", pairs))
    x, y = rows_and_colours(orc, str(tmp_path / "merged_halves.bxi")), rows_and_colours(orc, str(tmp_path / "collapsed_merge.bxi"))
    assert x[0] == y[0] and len(x[0]) == 39 and np.array_equal(x[1], y[1]) and x[1].any()
