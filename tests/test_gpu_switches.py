"""Every switch of cid_switches.def picks another kernel, template instance or host pipeline, and none of them may change a result:
each path a switch reaches, against the oracle (oracle/orc.py) or zlib and against the default path where the two share an input.

  a. upload_chunk_bytes: the double-buffered host-input pipeline of cid_search_count at chunks of 64 .. 192 k-mers, budgets below one
     k-mer (a chunk is then one tile of 64), batches on and around the chunk boundaries; a borrowed stream; a group of two ranks.
  b. inflate_wave / inflate_lanes: k_bgzf_inflate_wave and k_bgzf_inflate<1, 2, 4, 8> over every block type, and batches beyond
     twice each kernel's grid cap (the retry kernel's too), where every workgroup decodes member after member out of the same LDS.
  c. kmerset_dedupe / kmerset_crowded_at / kmerset_msd_sort / kmerset_target / kmerset_slice_mb: how the set's sort routes runs among
     its kernels, the targeted order, the slices of reads over the copy stream.
  d. order_bits: cid_kmerset_order_for_index is a STABLE sort of the set by its key, restated here from the oracle's hash.
  e. pin_staging / dense_report_bytes / COLORID_SYNC: the unpinned copies, one read per dense slice, the host's ways of waiting."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from test_gpu_fastq import fastq_text as records_text, line_loop_records
from test_gpu_inflate import bgzf_member, fastq_text, inflate
from test_gpu_kmerset_target import assert_target_order, rand_seq
from test_gpu_readid import pack_reads, sample_reads
from util import plant, random_index, random_kmers, synth_fastq_records, to_hip_index

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ACGT = np.frombuffer(b"ACGT", np.uint8)
OUTPUTS = ("hits", "n_unique", "sum_unique_freq", "unique_colour")


def _same(want, got, what):
    for w, g, name in zip(want, got, OUTPUTS):
        if w is not None and g is not None:
            assert np.array_equal(w, g), (what, name)


# ---------------------------------------------------------------------------------------------- a. host-chunked search

@pytest.mark.timeout(600)
@pytest.mark.parametrize("n_colors", [32, 256, 512, 1024])          # rows of 4, 32, 64 and 128 bytes of colour bits
@pytest.mark.parametrize("k", [21, 31, 40])
def test_host_chunked_search_equals_the_oracle(orc, hip_ctx, tune, k, n_colors):
    """budgets of 64, 128 and 192 k-mers per chunk, and 0, 1, k + 7 bytes (a chunk of one tile); batches of none, one, around a tile,
    around two chunks and of five chunks and a bit (both buffers reused behind ev_done); freq absent and present; each output left out"""
    rng = np.random.default_rng(k * 1000 + n_colors)
    oix = random_index(orc, rng, 20_011, 3, k, n_colors, density=0.2, zero_row_frac=0.1)
    kmers = random_kmers(rng, 5 * 192 + 17, k)
    plant(oix, rng, kmers, frac=0.6, max_colours=3)
    freq = rng.integers(1, 1000, size=len(kmers)).astype(np.uint32)
    hx = to_hip_index(hip_ctx, oix)
    for budget, c in ((64 * (k + 8), 64), (128 * (k + 8), 128), (192 * (k + 8), 192), (0, 64), (1, 64), (k + 7, 64)):
        tune("upload_chunk_bytes", budget)
        for n in sorted({0, 1, 63, 64, 65, 2 * c - 1, 2 * c, 2 * c + 1, 5 * c + 17}):
            km, fq = kmers[:n], freq[:n]
            want = oix.search_count(km, fq.astype(np.uint64))
            _same(want, hx.search_count(km, fq), (budget, n, "freq"))
            _same(oix.search_count(km, None), hx.search_count(km, None), (budget, n, "no freq"))
            for unique, colour in ((False, False), (True, False), (False, True)):
                got = hx.search_count(km, fq, want_unique=unique, want_unique_colour=colour)
                assert (got[1] is None) == (not unique) and (got[3] is None) == (not colour)
                _same(want, got, (budget, n, unique, colour))
        assert want[0].sum() > 0
    hx.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k,n_colors", [(31, 256), (40, 1024)])
def test_host_chunked_search_on_a_borrowed_stream_and_a_group(orc, hip_ctx, tune, k, n_colors):
    """a borrowed stream keeps everything on it (one chunk whatever the budget); two ranks on device 0 chunk their shards each"""
    import torch

    import colorid_amd
    rng = np.random.default_rng(k + n_colors)
    oix = random_index(orc, rng, 30_011, 4, k, n_colors, density=0.2, zero_row_frac=0.1)
    kmers = random_kmers(rng, 5 * 64 + 17, k)
    plant(oix, rng, kmers, frac=0.6, max_colours=3)
    freq = rng.integers(1, 1000, size=len(kmers)).astype(np.uint32)
    sizes = (0, 1, 2, 65, 129, 257, len(kmers))
    want = {n: oix.search_count(kmers[:n], freq[:n].astype(np.uint64)) for n in sizes}
    hx = to_hip_index(hip_ctx, oix)
    stream = torch.cuda.Stream(device=0)
    for budget in (0, 64 * (k + 8)):
        tune("upload_chunk_bytes", budget)
        for n in sizes:
            own = hx.search_count(kmers[:n], freq[:n])
            hip_ctx.set_stream(stream.cuda_stream)
            try:
                borrowed = hx.search_count(kmers[:n], freq[:n])
            finally:
                hip_ctx.set_stream(None)
            _same(want[n], own, (budget, n, "own stream"))
            _same(want[n], borrowed, (budget, n, "borrowed stream"))
    hx.close()
    g = colorid_amd.Group([0, 0])
    try:
        gx = colorid_amd.Index(g.ctxs[0], oix.m, oix.n_hash, oix.k, oix.n_colors)
        gx.put_dense(oix.rows())
        gx.finalize()
        g.replicate(gx)
        for budget in (0, 1, k + 7, 64 * (k + 8)):
            for cx in g.ctxs:
                cx.tune("upload_chunk_bytes", budget)      # (cid_group_ctx: the ranks' own contexts)
            for n in sizes:
                _same(want[n], g.search_count(kmers[:n], freq[:n]), (budget, n, "group"))
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- b. inflate paths and grid caps

INFLATE_PATHS = [(1, 0), (0, 0), (0, 1), (0, 2), (0, 4), (0, 8), (0, 3)]       # (inflate_wave, inflate_lanes); lanes 3 acts as 2


def _members_per_wave(wave, lanes, n):
    """what bgzf_inflate_launch takes: the wave kernel one member per wave, the one-lane kernel 1, 2, 4 or 8 (0: by the launch's size)"""
    if wave:
        return 1
    if lanes == 0:
        return 1 if n <= 1280 else 2
    return lanes if lanes in (1, 4, 8) else 2


@pytest.fixture(scope="module")
def block_corpus():
    """every block type (stored, fixed and dynamic Huffman codes), level and strategy, texts of 0 … 65536 bytes"""
    rng = np.random.default_rng(1)
    fq = fastq_text(rng, 3000)
    shapes = [(b"", 6), (b"A", 6), (b"ACGT" * 5, 1), (fq[:65280], 6), (fq[1000:66536], 9), (fq[:65280], 1), (fq[:40000], 0),
              (bytes(rng.integers(0, 256, 65536).astype(np.uint8)), 6), (bytes(rng.integers(0, 256, 70).astype(np.uint8)), 0),
              (b"\n" * 65536, 6), (b"AC" * 30000, 9), (b"ACGTTGCA" * 8000 + fq[:1000], 4),
              (bytes(rng.integers(0, 4, 65536).astype(np.uint8)), 6), (bytes(rng.choice([65, 67], size=50000, p=[0.999, 0.001]).astype(np.uint8)), 6)]
    texts = [t for t, _ in shapes]
    members = [bgzf_member(t, lv) for t, lv in shapes]
    for strat in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        for t in (fq[:65280], fq[70000:70100], b"N" * 3000 + fq[:5000]):
            texts.append(t); members.append(bgzf_member(t, 6, strat))
    texts.append(fq[:12345]); members.append(bgzf_member(fq[:12345], 6, extra_subfield=True))
    for _ in range(40):
        a = int(rng.integers(0, len(fq) - 65536)); n = int(rng.integers(1, 65537))
        texts.append(fq[a:a + n]); members.append(bgzf_member(fq[a:a + n], int(rng.integers(1, 10))))
    return texts, members


@pytest.fixture(scope="module")
def small_pool():
    """3 000 distinct members, most of them 20 .. 400 bytes of FASTQ text, 700 of them stored blocks (level 0: the retry kernel's)"""
    rng = np.random.default_rng(77)
    fq = fastq_text(rng, 8000)
    texts, members, stored = [], [], []
    for i in range(3000):
        n = int(rng.integers(20, 400)) if i % 40 else int(rng.integers(400, 9000))
        a = int(rng.integers(0, len(fq) - n))
        level = 0 if i < 700 else int(rng.integers(1, 10))
        texts.append(fq[a:a + n]); members.append(bgzf_member(fq[a:a + n], level)); stored.append(level == 0)
    order = rng.permutation(3000)
    return [texts[i] for i in order], [members[i] for i in order], [stored[i] for i in order]


def _tile(texts, members, n, extra=None):
    reps, rem = divmod(n, len(members))
    out = [members * reps + members[:rem], [len(t) for t in texts] * reps + [len(t) for t in texts[:rem]], b"".join(texts) * reps + b"".join(texts[:rem])]
    if extra is not None:
        out.append(extra * reps + extra[:rem])
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("wave,lanes", INFLATE_PATHS)
def test_inflate_paths_and_grid_caps_equal_zlib(block_corpus, small_pool, wave, lanes):
    import torch

    import colorid_amd
    cx = colorid_amd.Context(0)                 # (a context of its own: the big batches' buffers go with it)
    try:
        lib = cx.lib
        cx.tune("inflate_wave", wave)
        cx.tune("inflate_lanes", lanes)
        texts, members = block_corpus
        L = _members_per_wave(wave, lanes, 2)
        for n in sorted({1, L - 1, L + 1, 1281}):
            bm, bl, bt = _tile(texts, members, n)
            rc, out, bad, _ = inflate(lib, cx, bm, bl)
            assert rc == 0, (n, lib.cid_last_error())
            assert out == bt, n
        # a batch beyond twice the grid cap: every workgroup takes members in a second and later round
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        cap_groups = n_cu * 20 if wave else n_cu * 128
        lpw = _members_per_wave(wave, lanes, 2 * cap_groups * 8)
        n_big = 2 * cap_groups * lpw + 777
        ptexts, pmembers, pstored = small_pool
        bm, bl, bt, st = _tile(ptexts, pmembers, n_big, pstored)
        assert n_big > 2 * cap_groups * lpw, (n_cu, n_big)
        if wave:
            assert sum(st) > 2 * 256                # the retry kernel (k_bgzf_inflate<1>, at most 256 workgroups) strides too
        rc, out, bad, _ = inflate(lib, cx, bm, bl)
        assert rc == 0, (n_big, lib.cid_last_error())
        assert out == bt
        print(f"inflate_wave={wave} inflate_lanes={lanes}: n_cu {n_cu}, grid cap {cap_groups} workgroups x {lpw}, {n_big} members, "
              f"{sum(st)} stored")
        # one corrupt member past the cap is named, with its reason
        idx = max(i for i in range(n_big - 100, n_big) if not st[i])
        b = bytearray(bm[idx]); b[-6] ^= 0x01; bm[idx] = bytes(b)          # its CRC-32 field
        rc, out, bad, _ = inflate(lib, cx, bm, bl)
        assert rc == -1 and bad == idx and b"CRC-32" in lib.cid_last_error(), (rc, bad, idx, lib.cid_last_error())
        rc, out, bad, _ = inflate(lib, cx, bm[:idx] + bm[idx + 1:], bl[:idx] + bl[idx + 1:])   # and the context works on afterwards
        assert rc == 0
    finally:
        cx.close()


@pytest.fixture(scope="module")
def fastq_world(orc):
    rng = np.random.default_rng(31)
    genomes = [rand_seq(rng, 6000) for _ in range(4)]
    oix = random_index(orc, rng, 40_009, 3, 21, 130, density=0.02, zero_row_frac=0.2)
    for gi, g in enumerate(genomes):
        km = orc.Kmers(21)
        km.kmerize_vector(g, 1)
        for key in km.keys():
            oix.insert(gi * 7, key.tobytes())
    return rng, genomes, oix


@pytest.mark.timeout(300)
@pytest.mark.parametrize("switches", [{"inflate_wave": 0, "inflate_lanes": 4}, {"inflate_priority": 0, "fastq_inflate_beside": 0}])
def test_fastq_block_gzip_classify_on_other_inflate_paths(orc, fastq_world, switches):
    """cid_fastq's block-gzip front end with four members per wave of the one-lane kernel, and with the inflate on an ordinary queue
    behind the classifier: the oracle's classification of the quality-masked records"""
    import colorid_amd
    rng, genomes, oix = fastq_world
    recs = synth_fastq_records(np.random.default_rng(32), genomes, 3000, 150, lower_rate=0.0)
    text = records_text(recs)
    lines = line_loop_records(text)
    bases, so, r0 = pack_reads([[orc.qual_mask(s, q, 15)] for _, s, q in lines])
    w_rep, w_nk, w_st = oix.readid_counts(bases, so, r0, 1, 3)
    members, lens, pos = [], [], 0
    while pos < len(text):
        n = int(rng.choice([300, 5000, 30000, 65536]))
        members.append(bgzf_member(text[pos:pos + n], int(rng.integers(0, 10)))); lens.append(len(text[pos:pos + n]))
        pos += n
    members.append(bgzf_member(b"")); lens.append(0)
    ctx = colorid_amd.Context(0)                # (a context's inflate streams, and their priority, are made with its first reader)
    try:
        for name, value in switches.items():
            ctx.tune(name, value)
        hx = to_hip_index(ctx, oix)
        fr = colorid_amd.FastqReader(ctx, 1, 15)
        ids, nk, st, rows = [], [], [], []
        for i in range(0, len(members), 7):
            fr.push_bgzf(0, members[i:i + 7], lens[i:i + 7], last=(i + 7 >= len(members)))
            g_ids, g_nk, g_st, rs, col, cnt = fr.classify(hx, 1, 3)
            ids += g_ids; nk.append(g_nk); st.append(g_st)
            for r in range(len(g_ids)):
                row = np.zeros(oix.n_colors + 1, np.uint32)
                row[col[int(rs[r]):int(rs[r + 1])]] = cnt[int(rs[r]):int(rs[r + 1])]
                rows.append(row)
        assert ids == [ln[0] for ln in lines]
        assert np.array_equal(np.concatenate(nk), w_nk) and np.array_equal(np.concatenate(st), w_st)
        assert np.array_equal(np.array(rows), w_rep)
        assert w_rep[:, :oix.n_colors].sum() > 0
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- c. the k-mer set's sort routing

KMERSET_FLAVOURS = ["random", "deep", "repeats", "one_kmer", "ns", "mixed", "shared_prefix", "deep_errors"]


def kmerset_flavour(rng, flavour, k):
    """the inputs of test_gpu_kmerset_target.py's sort tests: spread keys, deep coverage, one k-mer, windows without k-mers, ..."""
    if flavour == "random":
        return [rand_seq(rng, 60_000), rand_seq(rng, 45_000)]
    if flavour == "deep":
        g = rand_seq(rng, 2000)
        return [g[s:s + 150] for s in rng.integers(0, len(g) - 150, 2000)]
    if flavour == "repeats":
        unit = np.frombuffer((rand_seq(rng, 7) * 9000)[:60_000], np.uint8).copy()
        hit = rng.random(len(unit)) < 0.002
        unit[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        return [unit.tobytes(), b"A" * 30_000, b"AC" * 10_000]
    if flavour == "one_kmer":
        return [b"A" * (k + 20_000)]
    if flavour == "shared_prefix":
        head = b"A" * min(14, k - 3)
        return [head + rand_seq(rng, k - len(head)) for _ in range(3500)] + [rand_seq(rng, 20_000)]
    if flavour == "deep_errors":
        g = np.frombuffer(rand_seq(rng, 3000), np.uint8)
        seqs = []
        for s0 in rng.integers(0, len(g) - 150, 3000):
            r = g[s0:s0 + 150].copy()
            hit = rng.random(150) < 0.01
            r[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            seqs.append(r.tobytes())
        return seqs
    if flavour == "ns":
        return [rand_seq(rng, 50_000, b"ACGTN"), b"N" * 5000, rand_seq(rng, 20_000, b"ACGTNNNN")]
    g = rand_seq(rng, 3000)
    return [rand_seq(rng, 40_000), b"T" * 9000, rand_seq(rng, 10_000, b"ACGTN")] + [g[s:s + 200] for s in rng.integers(0, 2800, 300)]


# (kmerset_dedupe, kmerset_crowded_at): at 0 every run is crowded; 2^31 - 1 wraps the 32-bit crowded_at * N of cid_partition.hpp /
# cid_rundedupe.hpp, so it may route differently — but never to another result
ROUTES = [(0, -1), (0, 0), (1, 0), (1, 1), (0, 64), (1, 64), (0, 2**31 - 1), (1, 2**31 - 1)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("flavour", KMERSET_FLAVOURS)
def test_kmerset_sort_routes_equal_the_oracle(orc, hip_ctx, tune, flavour, k):
    """every route through the MSD sort (kmerset_msd_min=1), in code order and targeted: the default's set is the oracle's (as a dict,
    by total count, in (first-row key, code) order when targeted), and every other route gives it array for array"""
    import colorid_amd
    tune("kmerset_msd_min", 1)
    tune("kmerset_target_small", 1)
    rng = np.random.default_rng(k * 31 + len(flavour))
    seqs = kmerset_flavour(rng, flavour, k)
    want = orc.Kmers(k)
    for s in seqs:
        want.kmerize_vector(s, 1)
    m = 50_021
    hx = colorid_amd.Index(hip_ctx, m, 3, k, 8)
    hx.finalize()

    def build(targeted):
        ks = colorid_amd.KmerSet(hip_ctx, k)
        if targeted:
            ks.set_target_index(hx)
        ks.add_seqs(seqs, 0)
        n = ks.finalize()
        km, cnt = ks.download()
        ks.close()
        assert n == len(cnt)
        return km, cnt

    base = {t: build(t) for t in (False, True)}
    for t, (km, cnt) in base.items():
        assert {bytes(km[i]): int(cnt[i]) for i in range(len(cnt))} == want.as_dict(), t
        assert int(cnt.sum()) == int(want.counts().sum())
    assert_target_order(orc, base[True][0], m)
    for dedupe, crowded in ROUTES:
        tune("kmerset_dedupe", dedupe)
        tune("kmerset_crowded_at", crowded)
        for t in (False, True):
            km, cnt = build(t)
            assert np.array_equal(km, base[t][0]) and np.array_equal(cnt, base[t][1]), (dedupe, crowded, t)
    tune("kmerset_dedupe", 1)
    tune("kmerset_crowded_at", -1)
    tune("kmerset_msd_sort", 0)                 # rocPRIM's LSD sort
    for t in (False, True):
        km, cnt = build(t)
        assert np.array_equal(km, base[t][0]) and np.array_equal(cnt, base[t][1]), ("lsd", t)
    tune("kmerset_msd_sort", 1)
    tune("kmerset_target", 0)                   # set_target_index is a no-op: the code-ordered set
    km, cnt = build(True)
    assert np.array_equal(km, base[False][0]) and np.array_equal(cnt, base[False][1])
    hx.close()


@pytest.mark.timeout(300)
def test_kmerset_reads_in_slices_of_one_mib(orc, hip_ctx, tune):
    """cid_kmerset_add_seqs with kmerset_slice_mb=1: 5 MiB of reads of 20 … 2 078 bases (k = 31: the longest a segment takes), every
    slice's last read ending exactly on the slice's boundary; a lower-case base in the last slice alone still refuses fastq mode"""
    import colorid_amd
    k, MiB = 31, 1 << 20
    tune("kmerset_slice_mb", 1)
    rng = np.random.default_rng(41)
    genome = rand_seq(rng, 200_000)
    lens, total = [], 0
    while total < 5 * MiB + 12_345:
        L = int(rng.integers(20, 2079))
        gap = (total // MiB + 1) * MiB - total          # to the next slice boundary (a slice ends with the first read that reaches it)
        if L >= gap:
            L = gap
        elif gap - L < 20:                              # (no read could fill what would be left)
            L = gap - 20 if gap - 20 >= 20 else gap
        lens.append(L)
        total += L
    seqs = [genome[s:s + L] for s, L in zip(rng.integers(0, len(genome) - 2100, len(lens)), lens)]
    ends = np.cumsum(lens)
    assert all(e in set(ends.tolist()) for e in range(MiB, 5 * MiB + 1, MiB)) and max(lens) <= 2078 and min(lens) >= 20
    for mode in (0, 1):
        want = orc.Kmers(k)
        for s in seqs:
            if mode == 0:
                want.kmerize_vector(s, 1)
            else:
                want.kmerize_fq_read(s, b"I" * len(s), 0)
        ks = colorid_amd.KmerSet(hip_ctx, k)
        ks.add_seqs(seqs, mode)
        assert ks.finalize() == len(want)
        km, cnt = ks.download()
        assert {bytes(km[i]): int(cnt[i]) for i in range(len(cnt))} == want.as_dict(), mode
        assert int(cnt.sum()) == int(want.counts().sum())
        ks.close()
    assert ends[-2] >= 5 * MiB                          # the last read lies in the last slice
    ks = colorid_amd.KmerSet(hip_ctx, k)
    with pytest.raises(colorid_amd.CidError) as ei:
        ks.add_seqs(seqs[:-1] + [seqs[-1].lower()], 1)
    assert ei.value.code == -4 and "lower-case" in str(ei.value)
    ks.close()


# ---------------------------------------------------------------------------------------------- d. order_for_index

ORDER_INDICES = [(32, 0), (256, 0), (1024, 0), (256, 1)]     # (n_colors, hash variant): rows of 8, 32 and 128 bytes; v0.7's hash


def _decode(codes, k):
    """2-bit codes (A C G T = 0 1 2 3, first base in the high bits: code order is ASCII order) -> k ASCII bytes each"""
    out = np.zeros((len(codes), k), np.uint8)
    for i in range(k):
        out[:, i] = ACGT[((codes >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.int64)]
    return out


def _order_key(row0, bits, m, line_shift):
    return (row0 << np.uint64(bits)) // np.uint64(m) if bits else row0 >> np.uint64(line_shift)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [21, 31, 40, 64])
def test_order_for_index_is_a_stable_sort_by_the_key(orc, hip_ctx, tune, k):
    """the download after cid_kmerset_order_for_index is the code-ordered download sorted STABLY by row0 >> line_shift (order_bits 0)
    or (row0 << order_bits) // m, row0 the first hash's row; counts go with their k-mers; the search over the set is the oracle's"""
    import colorid_amd
    rng = np.random.default_rng(500 + k)
    genome = rand_seq(rng, 6000)
    reads = [genome[s:s + 150] for s in rng.integers(0, len(genome) - 150, 400)]
    want = orc.Kmers(k)
    for s in reads:
        want.kmerize_vector(s, 1)
    m = 60_013
    for n_colors, variant in ORDER_INDICES:
        oix = random_index(orc, rng, m, 3, k, n_colors, density=0.2, zero_row_frac=0.1)
        plant(oix, rng, want.keys(), frac=0.6, max_colours=3)
        hx = colorid_amd.Index(hip_ctx, m, 3, k, n_colors, hash_variant=variant)
        hx.put_dense(oix.rows())
        hx.finalize()
        _, rs = hx.device_matrix()
        line_shift = 0
        while (rs << line_shift) < 16:
            line_shift += 1
        h = orc.xxh3_v07 if variant else orc.xxh3
        row0, km_code = None, None
        for bits in (0, 1, 7, 16, 31, 32):
            tune("order_bits", bits)
            ks = colorid_amd.KmerSet(hip_ctx, k)
            ks.add_seqs(reads, 0)
            ks.finalize()
            km0, cnt0 = ks.download()
            if row0 is None:
                assert {bytes(km0[i]): int(cnt0[i]) for i in range(len(cnt0))} == want.as_dict()
                row0 = np.array([h(bytes(r), 0) % m for r in km0], np.uint64)
                km_code = km0
            assert np.array_equal(km0, km_code)
            order = np.argsort(_order_key(row0, bits, m, line_shift), kind="stable")
            ks.order_for_index(hx)
            km1, cnt1 = ks.download()
            assert np.array_equal(km1, km0[order]) and np.array_equal(cnt1, cnt0[order]), (n_colors, variant, bits)
            with orc.hash_variant(variant):
                w = oix.search_count(km1, cnt1.astype(np.uint64))
            _same(w, ks.search_count(hx), (n_colors, variant, bits))
            assert w[0].sum() > 0
            ks.close()
        hx.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("bits", [0, 16])
def test_order_codes_for_index_dev_without_counts(orc, hip_ctx, tune, bits):
    """cid_order_codes_for_index_dev on a set's device arrays, d_counts = NULL and not: the same stable sort of the codes"""
    import torch

    import colorid_amd
    tune("order_bits", bits)
    k, m = 31, 60_013
    rng = np.random.default_rng(71)
    genome = rand_seq(rng, 8000)
    ks = colorid_amd.KmerSet(hip_ctx, k)
    ks.add_seqs([genome[s:s + 150] for s in rng.integers(0, len(genome) - 150, 500)], 0)
    n = ks.finalize()
    km0, cnt0 = ks.download()
    hx = colorid_amd.Index(hip_ctx, m, 3, k, 256)
    hx.finalize()
    _, rs = hx.device_matrix()
    line_shift = 0
    while (rs << line_shift) < 16:
        line_shift += 1
    row0 = np.array([orc.xxh3(bytes(r), 0) % m for r in km0], np.uint64)
    order = np.argsort(_order_key(row0, bits, m, line_shift), kind="stable")
    d_codes, d_counts, nn = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    colorid_amd.hip.check(hip_ctx.lib.cid_kmerset_device_arrays(ks.h, C.byref(d_codes), C.byref(d_counts), C.byref(nn)))
    assert nn.value == n
    dev = torch.device("cuda", 0)
    codes_a = torch.full((n,), -1, dtype=torch.int64, device=dev)
    codes_b = torch.full((n,), -1, dtype=torch.int64, device=dev)
    counts_b = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib = hip_ctx.lib
    colorid_amd.hip.check(lib.cid_order_codes_for_index_dev(hip_ctx.h, hx.h, d_codes.value, None, n, codes_a.data_ptr(), None))
    colorid_amd.hip.check(lib.cid_order_codes_for_index_dev(hip_ctx.h, hx.h, d_codes.value, d_counts.value, n, codes_b.data_ptr(),
                                                            counts_b.data_ptr()))
    hip_ctx.synchronize()
    a = codes_a.cpu().numpy().view(np.uint64)
    assert np.array_equal(_decode(a, k), km0[order])
    assert np.array_equal(codes_b.cpu().numpy().view(np.uint64), a)
    assert np.array_equal(counts_b.cpu().numpy().view(np.uint32), cnt0[order])
    ks.close(); hx.close()


# ---------------------------------------------------------------------------------------------- e. staging, slicing, waiting

@pytest.fixture(scope="module")
def readid_world(orc, hip_ctx):
    rng = np.random.default_rng(61)
    n_colors, n_hash, k, m = 130, 3, 27, 50_021
    oix = random_index(orc, rng, m, n_hash, k, n_colors, density=0.03, zero_row_frac=0.05)
    genomes = [rand_seq(rng, 4000) for _ in range(5)]
    for gi, g in enumerate(genomes):
        km = orc.Kmers(k)
        km.kmerize_vector(g, 1)
        for key in km.keys():
            oix.insert(gi, key.tobytes())
            oix.insert(n_colors - 1 - gi, key.tobytes())
    hx = to_hip_index(hip_ctx, oix)
    yield oix, hx, genomes
    hx.close()


def _check_sparse(want, got):
    rs, col, cnt, nk, st = got
    assert np.array_equal(nk, want[1]) and np.array_equal(st, want[2])
    rows, cols = np.nonzero(want[0])
    assert np.array_equal(rs, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(want[0])))]).astype(np.uint64))
    assert np.array_equal(col, cols.astype(np.uint32)) and np.array_equal(cnt, want[0][rows, cols])


@pytest.mark.timeout(300)
def test_unpinned_staging_equals_the_oracle(orc, hip_ctx, tune, readid_world):
    """pin_staging 1 and 0 (the copies straight from the caller's pageable memory): readid_count, _sparse, _resident, a striped index's
    read_id and cid_bgzf_inflate give the oracle's (zlib's) results either way"""
    import torch

    import colorid_amd
    oix, hx, genomes = readid_world
    rng = np.random.default_rng(62)
    reads = sample_reads(orc, rng, genomes, 500, 150, True)
    bases, so, r0 = pack_reads(reads)
    want = oix.readid_counts(bases, so, r0, 1, 3)
    assert want[0][:, :oix.n_colors].sum() > 0
    fq = fastq_text(rng, 2000)
    texts = [fq[i:i + 30000] for i in range(0, len(fq), 30000)]
    members = [bgzf_member(t, 1 + i % 9) for i, t in enumerate(texts)]
    dev = torch.device("cuda", 0)
    d_bases = torch.from_numpy(bases.copy()).to(dev)
    n = len(reads)
    for pin in (1, 0):
        tune("pin_staging", pin)
        rep, nk, st = hx.readid_count(bases, so, r0, 1, 3)
        assert np.array_equal(st, want[2]) and np.array_equal(nk, want[1]) and np.array_equal(rep, want[0]), pin
        _check_sparse(want, hx.readid_count_sparse(bases, so, r0, 1, 3))
        t_rep = torch.full((n, oix.n_colors + 1), 77, dtype=torch.int32, device=dev)
        t_nk = torch.full((n,), 77, dtype=torch.int32, device=dev)
        t_st = torch.full((n,), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        hx.readid_count_resident(d_bases.data_ptr(), so, r0, 1, 3, t_rep.data_ptr(), t_nk.data_ptr(), t_st.data_ptr())
        hip_ctx.synchronize()
        assert np.array_equal(t_st.cpu().numpy(), want[2]) and np.array_equal(t_nk.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(t_rep.cpu().numpy().view(np.uint32), want[0])
        rc, out, bad, _ = inflate(hip_ctx.lib, hip_ctx, members, [len(t) for t in texts])
        assert rc == 0 and out == fq, (pin, hip_ctx.lib.cid_last_error())
        g = colorid_amd.Group([0, 0])
        try:
            for cx in g.ctxs:
                cx.tune("pin_staging", pin)
            stp = g.stripes(oix.m, oix.n_hash, oix.k, oix.n_colors)
            rows = oix.rows()
            ids = np.nonzero(rows.any(axis=1))[0].astype(np.uint64)
            stp.put_rows(ids, np.ascontiguousarray(rows[ids.astype(np.int64)], np.uint32))
            stp.finalize()
            _check_sparse(want, stp.readid_count_sparse(bases, so, r0, 1, 3))
        finally:
            g.close()


@pytest.mark.timeout(120)
def test_dense_report_of_one_read_per_slice(orc, tune, readid_world):
    """dense_report_bytes=1, below one report row: cid_readid_count takes the batch one read per launch"""
    oix, hx, genomes = readid_world
    rng = np.random.default_rng(64)
    reads = sample_reads(orc, rng, genomes, 150, 150, True)
    bases, so, r0 = pack_reads(reads)
    want = oix.readid_counts(bases, so, r0, 1, 3)
    tune("dense_report_bytes", 1)
    rep, nk, st = hx.readid_count(bases, so, r0, 1, 3)
    assert np.array_equal(st, want[2]) and np.array_equal(nk, want[1]) and np.array_equal(rep, want[0])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["spin", "yield", "block"])
def test_sync_modes_in_a_fresh_process(orc, tmp_path, readid_world, mode):
    """COLORID_SYNC is process-wide and the first context decides: a search and a read_id in a child of its own per value"""
    oix, hx, genomes = readid_world
    rng = np.random.default_rng(65)
    kmers = random_kmers(rng, 3000, oix.k)
    freq = rng.integers(1, 50, size=len(kmers)).astype(np.uint32)
    sw = oix.search_count(kmers, freq.astype(np.uint64))
    reads = sample_reads(orc, rng, genomes, 200, 150, True)
    bases, so, r0 = pack_reads(reads)
    rep, nk, st = oix.readid_counts(bases, so, r0, 1, 3)
    case = str(tmp_path / "sync_case.npz")
    np.savez(case, rows=oix.rows(), kmers=kmers, freq=freq, hits=sw[0], nu=sw[1], sf=sw[2], uc=sw[3], bases=bases, so=so, r0=r0, rep=rep,
             nk=nk, st=st)
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import colorid_amd
z = np.load({case!r})
ctx = colorid_amd.Context(0)
hx = colorid_amd.Index(ctx, {oix.m}, {oix.n_hash}, {oix.k}, {oix.n_colors})
hx.put_dense(z['rows']); hx.finalize()
for name, g in zip(('hits', 'nu', 'sf', 'uc'), hx.search_count(z['kmers'], z['freq'])):
    assert np.array_equal(g, z[name]), name
rep, nk, st = hx.readid_count(z['bases'], z['so'], z['r0'], 1, 3)
assert np.array_equal(rep, z['rep']) and np.array_equal(nk, z['nk']) and np.array_equal(st, z['st'])
print('sync ok')
"""
    env = dict(os.environ, COLORID_SYNC=mode)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "sync ok" in p.stdout, p.stderr[-2000:]
