"""cid_bgzf_deflate_segments: several independent texts as block-gzip members in one call, no member spanning two of them.  The yardstick is
the contiguous coder itself: segment s's members are byte for byte what cid_bgzf_deflate (matches = 0) / cid_bgzf_deflate_lz (matches = 1)
returns for that segment's text alone; every member is also read back by zlib on its own."""
import struct
import zlib

import numpy as np
import pytest

import colorid_amd
from colorid_amd._lib import CID_ERR_INVALID
from colorid_amd.hip import bgzf_deflate

pytestmark = pytest.mark.gpu

BLOCK = 65280
LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 65279, 65280, 65281, 0, 130560, 130561, 3]
STORED = 9                                                                        # the segment of 65 281 random bytes: two stored members


def fastq_like(rng, n):
    """n bytes of records whose header lines repeat (the LZ coder finds matches) over four-letter sequences and a narrow quality range"""
    out = bytearray()
    i = int(rng.integers(1000))
    while len(out) < n:
        L = int(rng.integers(30, 151))
        out += b"@instrument:run:flowcell:1:%d some description\n" % i
        out += bytes(rng.choice(list(b"ACGT"), size=L).astype(np.uint8)) + b"\n+\n" + bytes(rng.integers(35, 74, L).astype(np.uint8)) + b"\n"
        i += 1
    return bytes(out[:n])


def members_of(blob, member_len):
    at, out = 0, []
    for n in member_len:
        out.append(blob[at:at + int(n)])
        at += int(n)
    assert at == len(blob)
    return out


def check_member(m, piece):
    """the member's own fields and zlib's reading of it, alone"""
    assert m[:4] == b"\x1f\x8b\x08\x04" and m[10:16] == b"\x06\x00BC\x02\x00"
    assert struct.unpack("<H", m[16:18])[0] == len(m) - 1                         # BSIZE
    crc, isize = struct.unpack("<II", m[-8:])
    assert isize == len(piece) and 0 < isize <= BLOCK and crc == zlib.crc32(piece)
    d = zlib.decompressobj(31)
    assert d.decompress(m) == piece and d.eof and not d.unused_data


def check_segments(ctx, segments, matches, compare):
    """compare: the segments whose members are set against the contiguous call's, byte for byte (every segment: counts, fields, zlib)"""
    blob, member_len, first = ctx.bgzf_deflate_segments(segments, matches=matches)
    assert len(blob) <= ctx.lib.cid_bgzf_deflate_segments_bound(sum(len(s) for s in segments), len(segments))
    members = members_of(blob, member_len)
    assert int(first[0]) == 0 and int(first[-1]) == len(members)
    for s, text in enumerate(segments):
        mine = members[int(first[s]):int(first[s + 1])]
        assert len(mine) == (len(text) + BLOCK - 1) // BLOCK, s                   # a zero-length segment: no member
        for k, m in enumerate(mine):
            check_member(m, text[k * BLOCK:(k + 1) * BLOCK])
        if s in compare:
            want, want_len = bgzf_deflate(ctx, text, matches=matches)
            assert b"".join(mine) == want and [len(m) for m in mine] == want_len.tolist(), (s, len(text))
    return blob, members


@pytest.mark.parametrize("matches", [False, True])
def test_every_segment_is_the_contiguous_call_on_its_text(hip_ctx, matches):
    rng = np.random.default_rng(31)
    lengths = LENGTHS + rng.integers(0, 5001, 40).tolist()
    segments = [fastq_like(rng, n) for n in lengths]
    segments[STORED] = bytes(rng.integers(0, 256, lengths[STORED]).astype(np.uint8))
    blob, members = check_segments(hip_ctx, segments, matches, set(range(len(segments))))
    stored = members[sum((n + BLOCK - 1) // BLOCK for n in lengths[:STORED]):][:2]
    assert [len(m) for m in stored] == [BLOCK + 31, 1 + 31]                       # incompressible: the stored form, text + 31
    if matches:                                                                   # the LZ coder did find matches in this text
        plain = hip_ctx.bgzf_deflate_segments(segments, matches=False)[0]
        assert len(blob) < len(plain)
    assert hip_ctx.bgzf_deflate_segments(segments, matches=matches)[0] == blob    # a function of the texts alone


@pytest.mark.parametrize("matches", [False, True])
def test_more_segments_than_a_scan_tile(hip_ctx, matches):
    """2 500 segments of 0 .. 40 bytes: the scans over the segments and the one over the members' lengths cross a tile of 2 048 elements"""
    rng = np.random.default_rng(32)
    lengths = rng.integers(1, 41, 2500)
    lengths[rng.permutation(2500)[:440]] = 0                                      # about a fifth are empty; 2 060 members are left
    lengths = lengths.tolist()
    assert len(lengths) > 2048 and sum(1 for n in lengths if n) > 2048
    text = fastq_like(rng, sum(lengths))
    at, segments = 0, []
    for n in lengths:
        segments.append(text[at:at + n])
        at += n
    check_segments(hip_ctx, segments, matches, set(rng.choice(2500, 40, replace=False).tolist()))


def test_empty_inputs(hip_ctx):
    assert hip_ctx.bgzf_deflate_segments([])[:2][0] == b""
    blob, member_len, first = hip_ctx.bgzf_deflate_segments([b"", b"", b""])
    assert blob == b"" and len(member_len) == 0 and first.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("matches", [False, True])
def test_the_bound_holds_and_a_byte_less_is_refused(hip_ctx, matches):
    """segments of one byte: a member of 32 bytes each (the stored form, text + 31), so the members take exactly
    cid_bgzf_deflate_segments_bound — that much room is never refused, one byte less is, and the call says how much it needs"""
    rng = np.random.default_rng(33)
    segments = [bytes([int(b)]) for b in rng.integers(0, 256, 70)] + [b""] + [fastq_like(rng, 3 * BLOCK + 5)]
    n_text = sum(len(s) for s in segments)
    bound = hip_ctx.lib.cid_bgzf_deflate_segments_bound(n_text, len(segments))
    assert bound == n_text + 31 * (n_text // BLOCK + len(segments))
    blob, member_len, first = hip_ctx.bgzf_deflate_segments(segments, matches=matches, cap=bound)
    assert len(blob) <= bound and len(member_len) == 70 + 4
    with pytest.raises(colorid_amd.CidError) as e:
        hip_ctx.bgzf_deflate_segments(segments, matches=matches, cap=len(blob) - 1)
    assert e.value.code == CID_ERR_INVALID and str(len(blob)) in str(e.value)
    assert hip_ctx.bgzf_deflate_segments(segments, matches=matches, cap=len(blob))[0] == blob
    ones = segments[:70]                                                          # the bound met exactly
    tight = hip_ctx.lib.cid_bgzf_deflate_segments_bound(70, 70)
    blob1 = hip_ctx.bgzf_deflate_segments(ones, matches=matches, cap=tight)[0]
    assert len(blob1) == tight == 70 * 32
    with pytest.raises(colorid_amd.CidError) as e:
        hip_ctx.bgzf_deflate_segments(ones, matches=matches, cap=tight - 1)
    assert e.value.code == CID_ERR_INVALID
