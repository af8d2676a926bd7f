"""cid_bgzf_deflate: block-gzip members written on the GPU (one wave per member: histogram, length-limited Huffman code, literals coded in
parallel; stored when that is not smaller) against zlib — zlib.decompressobj(31) over the members checks the codes, the CRC-32 and the
ISIZE of every one; the framing ("BC", BSIZE) is checked here, and cid_bgzf_inflate reads the members back."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from colorid_amd._lib import CID_ERR_INVALID
from deflate_props import BLOCK, gunzip_members, illumina_fastq, literal_code_lengths, split_members, unlimited_huffman_depth
from test_gpu_inflate import inflate

pytestmark = pytest.mark.gpu


def fibonacci_text(rng):
    """all 256 byte values with Fibonacci-like counts: 246 values once each (with the end-of-block a subtree of 247 leaves, at least 8
    deep), then 10 values each counted one more than the whole tree below the one before it, so that whichever way ties fall the
    Huffman tree is a chain of 10 above that subtree: 18 levels unlimited, 35 710 bytes"""
    below = [256 - 10 + 1]                                                       # the weight of the tree so far
    counts = []
    for i in range(10):
        counts.append(below[max(i - 1, 0)] + 1)
        below.append(below[-1] + counts[-1])
    counts = [1] * (256 - 10) + counts
    values = rng.permutation(256)
    text = np.repeat(values.astype(np.uint8), counts)
    rng.shuffle(text)
    return text.tobytes()


def _texts():
    rng = np.random.default_rng(77)
    fq = illumina_fastq(rng, 200_000)
    return {
        "empty": b"",
        "one_byte": b"A",
        "fastq_65279": fq[:BLOCK - 1],
        "fastq_65280": fq[:BLOCK],
        "fastq_65281": fq[:BLOCK + 1],
        "one_value_65280": b"G" * BLOCK,
        "random_70000": bytes(rng.integers(0, 256, 70_000).astype(np.uint8)),
        "fibonacci": fibonacci_text(rng),
        "fastq_200k": fq,
    }


TEXTS = _texts()


@pytest.mark.parametrize("name", list(TEXTS))
def test_deflate_round_trip(hip_ctx, name):
    from colorid_amd.hip import bgzf_deflate
    text = TEXTS[name]
    lib = hip_ctx.lib
    blob, member_len = bgzf_deflate(hip_ctx, text)
    n = (len(text) + BLOCK - 1) // BLOCK
    assert len(member_len) == n
    pieces = [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]
    print(f"{name}: {len(text)} bytes -> {len(blob)} in {n} members {member_len.tolist()}")
    # zlib reads every member and gives the text back
    got = gunzip_members(blob)
    assert got == pieces
    # framing: BC, BSIZE + 1 == the member's length == member_len[i]; never longer than stored
    members = split_members(blob)
    assert [len(m) for m in members] == member_len.tolist()
    for m, p in zip(members, pieces):
        assert len(m) <= len(p) + 31
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(p) & 0xFFFFFFFF, len(p))
    assert len(blob) <= lib.cid_bgzf_deflate_bound(len(text))
    if name == "random_70000":
        assert [len(m) for m in members] == [len(p) + 31 for p in pieces]          # stored: nothing to gain on uniform bytes
        assert all(m[18] == 0x01 for m in members)                                # BFINAL, BTYPE 00
    if name in ("fastq_200k", "fastq_65280", "one_value_65280", "fibonacci"):
        assert all((m[18] & 7) == 0b101 for m in members)                         # BFINAL, dynamic Huffman
    if name == "fibonacci":                                                       # the case is what it claims: the plain tree is deeper than
        assert unlimited_huffman_depth(text) > 15                                 # DEFLATE allows, and the limited code reaches the limit
        lens, _ = literal_code_lengths(members[0])
        assert max(lens) == 15 and sum(2.0 ** -l for l in lens if l) == 1.0
    if name == "fastq_200k":
        assert n == 4 and len(blob) < len(text)
    if name == "one_value_65280":
        assert len(blob) < BLOCK // 7                                             # one bit per literal
    # the device's own inflate reads them back
    if n:
        rc, out, bad, _ = inflate(lib, hip_ctx, members, [len(p) for p in pieces])
        assert rc == 0, lib.cid_last_error()
        assert out == text
    # deterministic: a second call gives the same bytes
    blob2, member_len2 = bgzf_deflate(hip_ctx, text)
    assert blob2 == blob and member_len2.tolist() == member_len.tolist()


@pytest.mark.parametrize("name", list(TEXTS))
def test_deflate_dev_equals_host_form(hip_ctx, name):
    import torch
    from colorid_amd.hip import bgzf_deflate
    text = TEXTS[name]
    lib = hip_ctx.lib
    blob, member_len = bgzf_deflate(hip_ctx, text)
    cap = lib.cid_bgzf_deflate_bound(len(text))
    n = (len(text) + BLOCK - 1) // BLOCK
    d_text = torch.from_numpy(np.frombuffer(text + b"\0" * 16, np.uint8).copy()).cuda()
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nm = C.c_size_t(99)
    rc = lib.cid_bgzf_deflate_dev(hip_ctx.h, d_text.data_ptr(), len(text), d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    assert rc == 0, lib.cid_last_error()
    assert lib.cid_ctx_synchronize(hip_ctx.h) == 0
    assert nm.value == n
    total = int(d_total.cpu()[0])
    assert total == len(blob)
    assert d_out.cpu().numpy()[:total].tobytes() == blob
    assert d_len.cpu().numpy()[:n].astype(np.uint32).tolist() == member_len.tolist()
    # a buffer below the bound is refused before anything is queued
    if len(text):
        assert lib.cid_bgzf_deflate_dev(hip_ctx.h, d_text.data_ptr(), len(text), d_out.data_ptr(), cap - 1, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm)) == CID_ERR_INVALID


def test_deflate_host_buffer_too_small(hip_ctx):
    lib = hip_ctx.lib
    text = np.frombuffer(TEXTS["random_70000"], np.uint8)
    out = np.zeros(70_000, np.uint8)
    ln = np.zeros(2, np.uint32)
    nb, nm = C.c_size_t(0), C.c_size_t(0)
    rc = lib.cid_bgzf_deflate(hip_ctx.h, text.ctypes.data, len(text), out.ctypes.data, out.size, C.byref(nb), ln.ctypes.data, C.byref(nm))
    assert rc == CID_ERR_INVALID and nb.value == 70_000 + 62 and b"70062" in lib.cid_last_error()
    assert not out.any()
