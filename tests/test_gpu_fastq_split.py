"""cid_fastq_split: the records of a classified step dealt into bins, every bin's block-gzip members as one byte range, against the
restatement of the reference's read_filter that cid_fastq_filter's tests use (the lines as lines() gives them, a record written as
`header\\nsequence\\n+\\nquality\\n`) — applied once per bin — and against cid_fastq_filter itself where the two must agree byte for byte."""
import ctypes as C
import struct

import numpy as np
import pytest

import colorid_amd
from colorid_amd._lib import CID_ERR_INVALID, CID_ERR_STATE
from test_gpu_fastq import line_loop_records, world  # noqa: F401  (the toy index of the front end's tests)
from test_gpu_fastq_filter import gunzip, make_text

pytestmark = pytest.mark.gpu

DROP = 0xFFFFFFFF
BLOCK = 65280


def restated(records, bins, b):
    return b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, s, q), k in zip(records, bins) if k == b)


def member_sizes(blob):
    """(the member's bytes, its ISIZE) of every member of a range, walked by the BSIZE fields"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 14] == b"BC"
        n = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        out.append((n, struct.unpack("<I", blob[at + n - 4:at + n])[0]))
        at += n
    assert at == len(blob)
    return out


def one_step(hip_ctx, hx, texts):
    fr = colorid_amd.FastqReader(hip_ctx, len(texts), 0)
    fr.keep_steps()
    for f, t in enumerate(texts):
        fr.push_text(f, t, last=True)
    return fr, len(fr.classify(hx, 1, 3)[0])


@pytest.mark.parametrize("n_files", [1, 2])
def test_every_bin_is_the_restated_read_filter_of_its_records(hip_ctx, world, n_files):
    oix, hx, genomes = world
    rng = np.random.default_rng(41 + n_files)
    texts = [make_text(rng, genomes, 300, f + 1, last_newline=(f == 1)) for f in range(n_files)]
    records = [line_loop_records(t) for t in texts]
    assert all(len(r) == 300 for r in records)
    fr = colorid_amd.FastqReader(hip_ctx, n_files, 0)
    fr.keep_steps()
    n_bins = 6                                                                    # bin 4: nobody's
    got = [[b""] * n_bins for _ in range(n_files)]
    all_bins, reads, done = [], np.zeros(n_bins, np.uint64), 0
    for part in range(2):                                                        # two pushes, cut inside a record
        for f in range(n_files):
            cut = len(texts[f]) * 2 // 5 + 11 * f
            fr.push_text(f, texts[f][:cut] if part == 0 else texts[f][cut:], last=(part == 1))
        n = len(fr.classify(hx, 1, 3)[0])
        assert n
        bins = rng.choice(np.array([0, 1, 2, 3, 5, DROP], np.uint32), n)
        if done <= 150 < done + n:
            bins[150 - done] = 2                                                  # the 70 000-base record is kept: bin 2 takes several members
        all_bins += bins.tolist()
        for f in range(n_files):
            blob, off, bin_reads, n_members = fr.split(bins, n_bins, f)
            assert int(off[0]) == 0 and int(off[-1]) == len(blob) and np.all(np.diff(off.astype(np.int64)) >= 0)
            assert bin_reads.tolist() == [int(np.sum(bins == b)) for b in range(n_bins)]
            assert int(off[4]) == int(off[5])                                     # the bin nobody has: an empty range
            total_members = 0
            for b in range(n_bins):
                part_blob = blob[int(off[b]):int(off[b + 1])]
                text = gunzip(part_blob)
                sizes = member_sizes(part_blob)
                assert [t for _, t in sizes] == [min(BLOCK, len(text) - k * BLOCK) for k in range(len(sizes))]   # cut from the bin's start
                total_members += len(sizes)
                got[f][b] += text
            assert total_members == n_members
            if f == 0:
                reads += bin_reads
        blob, off, bin_reads, n_members = fr.split(np.full(n, DROP, np.uint32), n_bins, 0)   # all dropped
        assert (blob, n_members) == (b"", 0) and not off.any() and not bin_reads.any()
        done += n
    assert done == 300 and reads.tolist() == [all_bins.count(b) for b in range(n_bins)]
    for f in range(n_files):
        for b in range(n_bins):
            assert got[f][b] == restated(records[f], all_bins, b), (f, b)
    assert any(len(got[0][b]) > BLOCK for b in range(n_bins))                     # the 70 000-base record: a bin of several members
    fr.close()


def test_members_are_cut_from_the_start_of_each_bin(hip_ctx, world):
    """one bin of exactly 65 280 bytes of text (one member), one of 65 281 (two, the second of one byte), their records interleaved"""
    oix, hx, genomes = world
    rng = np.random.default_rng(43)

    def record(name, L):
        return name + b"\n" + bytes(rng.choice(list(b"ACGT"), size=L).astype(np.uint8)) + b"\n+\n" + bytes(rng.integers(35, 74, L).astype(np.uint8)) + b"\n"
    # "@r%05d" is 7 bytes: a record of 12 + 2 L bytes; 307 of 212 and one of 196 make 65 280.  "@r%06d": 13 + 2 L, the last one 197
    a = [record(b"@r%05d" % i, 100 if i < 307 else 92) for i in range(308)]
    b = [record(b"@r%05d" % i, 100) for i in range(307)] + [record(b"@r%06d" % 307, 92)]
    assert sum(map(len, a)) == BLOCK and sum(map(len, b)) == BLOCK + 1
    text = b"".join(x + y for x, y in zip(a, b))
    fr, n = one_step(hip_ctx, hx, [text])
    assert n == 616
    blob, off, bin_reads, n_members = fr.split(np.tile(np.array([2, 0], np.uint32), 308), 3, 0)
    assert bin_reads.tolist() == [308, 0, 308] and n_members == 3
    first, second = blob[int(off[0]):int(off[1])], blob[int(off[2]):int(off[3])]
    assert gunzip(first) == b"".join(b) and gunzip(second) == b"".join(a)
    assert [t for _, t in member_sizes(first)] == [BLOCK, 1] and [t for _, t in member_sizes(second)] == [BLOCK]
    fr.close()


@pytest.mark.parametrize("matches", [False, True])
def test_one_bin_is_cid_fastq_filter_byte_for_byte(hip_ctx, world, matches):
    """cid_fastq_filter is cid_fastq_split with one bin, so the first comparison holds a path against itself; the second holds it against
    the contiguous coder (cid_bgzf_deflate / cid_bgzf_deflate_lz of the restated text), which shares no layout code with the segment table"""
    from colorid_amd.hip import bgzf_deflate
    oix, hx, genomes = world
    rng = np.random.default_rng(44)
    text = make_text(rng, genomes, 300, 1, True)
    records = line_loop_records(text)
    fr, n = one_step(hip_ctx, hx, [text])
    assert n == 300
    fr.filter_matches(matches)
    for keep in (np.ones(n, np.uint8), (rng.random(n) < 0.5).astype(np.uint8)):
        want, want_members, want_kept = fr.filter(keep, 0)
        bins = np.where(keep != 0, 0, DROP).astype(np.uint32)
        blob, off, bin_reads, n_members = fr.split(bins, 1, 0)
        assert blob == want and (n_members, int(bin_reads[0])) == (want_members, want_kept) and off.tolist() == [0, len(want)]
        kept_text = restated(records, bins.tolist(), 0)
        if keep.all():                                                            # with the empty sequence and the 70 000-base record: several members
            assert n_members > 1 and records[7][1] == b"" and len(records[150][1]) == 70_000
        contiguous, member_len = bgzf_deflate(hip_ctx, kept_text, matches)
        assert blob == contiguous and n_members == len(member_len)
        bins3 = np.where(keep != 0, 1, DROP).astype(np.uint32)                    # the same records as bin 1 of 3
        blob3, off3, reads3, _ = fr.split(bins3, 3, 0)
        assert blob3 == want and off3.tolist() == [0, 0, len(want), len(want)] and reads3.tolist() == [0, want_kept, 0]
    if matches:                                                                   # the coder did change with the switch
        fr.filter_matches(False)
        assert fr.split(np.zeros(n, np.uint32), 1, 0)[0] == fr.filter(np.ones(n, np.uint8), 0)[0]
    fr.close()


def test_more_reads_and_more_bins_than_a_scan_tile(hip_ctx, world):
    """3 000 reads into 2 600 bins: the scan over the reads in output order and the two over the bins cross a tile of 2 048 elements"""
    oix, hx, genomes = world
    rng = np.random.default_rng(45)
    out = bytearray()
    for i in range(3000):
        L = int(rng.integers(30, 61))
        g = genomes[i % len(genomes)]
        a = int(rng.integers(0, len(g) - L))
        out += b"@q%d\n" % i + g[a:a + L] + b"\n+\n" + bytes(rng.integers(35, 74, L).astype(np.uint8)) + b"\n"
    text = bytes(out)
    records = line_loop_records(text)
    fr, n = one_step(hip_ctx, hx, [text])
    assert n == 3000
    n_bins = 2600
    bins = rng.permutation(n_bins).astype(np.uint32)[rng.integers(0, n_bins, n)]   # most bins hold 0 .. 2 reads, ids shuffled
    blob, off, bin_reads, n_members = fr.split(bins, n_bins, 0)
    counts = np.bincount(bins, minlength=n_bins)
    assert bin_reads.tolist() == counts.tolist() and n_members == int(np.sum(counts > 0)) and int(off[-1]) == len(blob)
    assert int(np.sum(counts == 0)) > 500 and int(np.sum(counts > 2)) > 100 and n > 2048 and n_bins > 2048
    by_bin = {}
    for r, b in enumerate(bins.tolist()):
        h, s, q = records[r]
        by_bin[b] = by_bin.get(b, b"") + h + b"\n" + s + b"\n+\n" + q + b"\n"
    for b in range(n_bins):
        assert gunzip(blob[int(off[b]):int(off[b + 1])]) == by_bin.get(b, b""), b
    fr.close()


def test_what_split_refuses(hip_ctx, world):
    oix, hx, genomes = world
    lib = hip_ctx.lib
    fr = colorid_amd.FastqReader(hip_ctx, 1, 0)
    with pytest.raises(colorid_amd.CidError) as e:                               # the reader keeps no steps
        fr.split(np.zeros(4, np.uint32), 2, 0)
    assert e.value.code == CID_ERR_STATE
    fr.keep_steps()
    with pytest.raises(colorid_amd.CidError) as e:                               # no step has ended
        fr.split(np.zeros(4, np.uint32), 2, 0)
    assert e.value.code == CID_ERR_STATE
    text = make_text(np.random.default_rng(46), genomes, 40, 1, True)
    fr.push_text(0, text, last=True)
    n = len(fr.classify(hx, 1, 3)[0])
    assert n == 40
    bins = (np.arange(n) % 3).astype(np.uint32)
    with pytest.raises(colorid_amd.CidError) as e:                               # no bins at all
        fr.split(bins, 0, 0)
    assert e.value.code == CID_ERR_INVALID
    bad = bins.copy()
    bad[17] = 3                                                                   # a bin id equal to n_bins
    with pytest.raises(colorid_amd.CidError) as e:
        fr.split(bad, 3, 0)
    assert e.value.code == CID_ERR_INVALID and "17" in str(e.value)
    # a buffer too short: the size the call needs comes back, nothing is written, and the same call with that much room succeeds
    out = np.full(64, 0xAB, np.uint8)
    off, reads = np.zeros(4, np.uint64), np.zeros(3, np.uint64)
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    args = lambda buf: (fr.h, bins.ctypes.data_as(C.c_void_p), 3, 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(nb), off.ctypes.data_as(C.c_void_p),
                        reads.ctypes.data_as(C.c_void_p), C.byref(nm))
    assert lib.cid_fastq_split(*args(out)) == CID_ERR_INVALID and nb.value > 64 and np.all(out == 0xAB)
    room = np.zeros(nb.value, np.uint8)
    assert lib.cid_fastq_split(*args(room)) == 0 and int(off[-1]) == nb.value == room.size
    records = line_loop_records(text)
    for b in range(3):
        assert gunzip(room[int(off[b]):int(off[b + 1])].tobytes()) == restated(records, bins.tolist(), b)
    fr.close()
