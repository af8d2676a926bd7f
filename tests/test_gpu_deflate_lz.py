"""cid_bgzf_deflate_lz: block-gzip members with LZ77 matches written on the GPU (tests/deflate_lz_props.py has the DEFLATE reader and the
rules).  Every case: check_lz_member per member, the bound, every member either cid_bgzf_deflate's byte for byte or strictly shorter,
and a second call gives the same bytes."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_props as P
from colorid_amd._lib import CID_ERR_INVALID
from deflate_lz_props import DIST_BASE, binned_fastq, check_lz_blob, check_lz_member, cut, matches_of
from deflate_props import BLOCK, split_members
from test_gpu_deflate import fibonacci_text

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the texts

def every_length_text(rng):
    """every match length 258 ... 3 once, the longest first: a fresh random segment of L bytes, two bytes that name L, the segment again,
    then a byte that differs from the one behind the first copy (and the byte before the second copy differs from the one before the
    first): the repeat is L bytes and no more"""
    out = []
    for L in range(258, 2, -1):
        seg = bytes(rng.integers(0, 256, L).astype(np.uint8))
        out.append(seg + bytes([L & 0xFF, 0x80 | (L >> 8)]) + seg + bytes([(L & 0xFF) ^ 0xFF]))
    return b"".join(out)


def distance_text(rng):
    """a random block repeated at exactly D bytes for every D at which a distance code begins, and 32 768: the short ones back to back
    in the first piece (filled up with random bytes), each of the six longest in a piece of its own"""
    short = b"".join((bytes(rng.integers(0, 256, D).astype(np.uint8)) * (2 + 300 // D + 1))[:2 * D + 300] for D in DIST_BASE if D <= 4097)
    assert len(short) < BLOCK
    pieces = [short + bytes(rng.integers(0, 256, BLOCK - len(short)).astype(np.uint8))]
    for D in [d for d in DIST_BASE if d > 4097] + [32768]:
        block = bytes(rng.integers(0, 256, D).astype(np.uint8))
        pieces.append((block * (BLOCK // D + 1))[:BLOCK])
    return b"".join(pieces)


def no_trigram_repeat_text(rng):
    """light value, heavy value, light, heavy, ...: every (light, heavy) pair of 240 x 16 values once, in a random order, so that no three
    bytes occur twice — and half the text is 16 values, which a Huffman code takes in 4 bits: worth coding, nothing to match"""
    values = rng.permutation(256).astype(np.uint8)
    light, heavy = values[:240], values[240:]
    pairs = np.array([(x, h) for x in light for h in heavy], np.uint8)
    text = pairs[rng.permutation(len(pairs))].reshape(-1).tobytes()
    grams = {text[i:i + 3] for i in range(len(text) - 2)}
    assert len(grams) == len(text) - 2
    return text


def _texts():
    rng = np.random.default_rng(2024)
    fq = P.illumina_fastq(rng, 200_000)
    binned = binned_fastq(rng, 200_000)
    fib = fibonacci_text(rng)
    once = bytes(rng.integers(0, 256, 600).astype(np.uint8))
    far = bytes(rng.integers(0, 256, 36_000).astype(np.uint8))
    record = binned_fastq(rng, 200)
    return {
        "empty": b"",
        "bytes_1": b"A", "bytes_2": b"AC", "bytes_3": b"ACG", "bytes_4": b"ACGT",
        "run_65280": b"G" * BLOCK, "run_65279": b"G" * (BLOCK - 1), "run_65281": b"G" * (BLOCK + 1),
        "every_length": every_length_text(rng),
        "distances": distance_text(rng),
        "repeat_beyond_window": far + far[:BLOCK - 36_000],                       # the only repeat lies 36 000 bytes back
        "second_piece_repeats_first": binned[:BLOCK] + binned[BLOCK - 1024:BLOCK] + fq[:30_000],
        "no_trigram_repeat": no_trigram_repeat_text(rng),
        "one_distance_symbol": once * 2,                                           # every repeat 600 bytes back
        "random_70000": bytes(rng.integers(0, 256, 70_000).astype(np.uint8)),
        "fibonacci_far_repeat": fib + fib[5000:7000],
        "record_x300": record * 300,
        "fastq_200k": fq,
        "binned_200k": binned,
    }


TEXTS = _texts()
_RESULTS = {}


def run_case(ctx, name):
    """-> (LZ members, today's members, tokens per member): checked once per text, shared by the tests that look closer"""
    if name in _RESULTS:
        return _RESULTS[name]
    from colorid_amd.hip import bgzf_deflate
    text = TEXTS[name]
    pieces = cut(text)
    blob, member_len = bgzf_deflate(ctx, text, matches=True)
    members, tokens = check_lz_blob(blob, member_len, pieces)
    assert len(blob) <= ctx.lib.cid_bgzf_deflate_bound(len(text))
    plain = split_members(bgzf_deflate(ctx, text)[0])
    assert len(plain) == len(members)
    for i, (m, q) in enumerate(zip(members, plain)):
        assert m == q or len(m) < len(q), f"{name}: member {i} is neither today's member nor shorter ({len(m)} against {len(q)} bytes)"
    blob2, member_len2 = bgzf_deflate(ctx, text, matches=True)
    assert blob2 == blob and member_len2.tolist() == member_len.tolist(), "a second call gives other bytes"
    n_match = sum(len(matches_of(t)) for t in tokens)
    print(f"{name}: {len(text)} bytes -> {len(blob)} with matches ({n_match} of them), {sum(len(q) for q in plain)} without; "
          f"{sum(m != q for m, q in zip(members, plain))} of {len(members)} members in the LZ form")
    _RESULTS[name] = (members, plain, tokens)
    return _RESULTS[name]


def deflate_dev(ctx, fn, text_array, text_bytes):
    """a _dev entry point over a host uint8 array that ends in 16 bytes of padding -> (d_out, member lengths [numpy], total)"""
    import torch
    lib = ctx.lib
    n = (text_bytes + BLOCK - 1) // BLOCK
    cap = lib.cid_bgzf_deflate_bound(text_bytes)
    d_text = torch.from_numpy(text_array).cuda()
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nm = C.c_size_t(99)
    rc = fn(ctx.h, d_text.data_ptr(), text_bytes, d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    assert rc == 0, lib.cid_last_error()
    assert lib.cid_ctx_synchronize(ctx.h) == 0
    assert nm.value == n
    del d_text
    return d_out, d_len.cpu().numpy()[:n].astype(np.int64), int(d_total.cpu()[0])


# ---------------------------------------------------------------------------------------------------------------- the cases

@pytest.mark.parametrize("name", list(TEXTS))
def test_members_keep_the_rules_and_never_lose_to_todays(hip_ctx, name):
    members, plain, tokens = run_case(hip_ctx, name)
    assert len(members) == (len(TEXTS[name]) + BLOCK - 1) // BLOCK


@pytest.mark.parametrize("name", ["bytes_3", "run_65281", "one_distance_symbol", "every_length", "fibonacci_far_repeat", "binned_200k"])
def test_dev_form_equals_host_form(hip_ctx, name):
    members, _, _ = run_case(hip_ctx, name)
    text = TEXTS[name]
    d_out, lens, total = deflate_dev(hip_ctx, hip_ctx.lib.cid_bgzf_deflate_lz_dev, np.frombuffer(text + b"\0" * 16, np.uint8).copy(), len(text))
    assert lens.tolist() == [len(m) for m in members] and total == int(lens.sum())
    assert d_out.cpu().numpy()[:total].tobytes() == b"".join(members)


def test_runs_end_0_1_and_2_bytes_behind_a_full_match(hip_ctx):
    for name in ("run_65280", "run_65279", "run_65281"):
        members, plain, tokens = run_case(hip_ctx, name)
        assert (258, 1) in tokens[0] or any(t[0] == 258 for t in matches_of(tokens[0]))
        assert all(d < l for l, d in matches_of(tokens[0])[:4])                     # overlapping copies: what a run of one byte needs
    assert len(run_case(hip_ctx, "run_65281")[0]) == 2 and len(TEXTS["run_65281"]) - BLOCK == 1


def test_lengths_257_and_258_both_occur(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "every_length")
    lengths = {l for t in tokens for l, d in matches_of(t)}
    print(f"every_length: {len(lengths)} distinct match lengths, {min(lengths)} .. {max(lengths)}")
    assert 257 in lengths and 258 in lengths                                        # 258 is symbol 285, 257 is 284 + 30


def test_distances_at_the_code_borders_and_beyond_the_window(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "distances")
    assert len(members) == 7
    print(f"distances: found {sorted({d for t in tokens for l, d in matches_of(t)})[:40]}")
    members, plain, tokens = run_case(hip_ctx, "repeat_beyond_window")
    assert not matches_of(tokens[0]) and members == plain                          # 36 000 bytes back is no source: today's (stored) member


def test_the_second_piece_inflates_alone(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "second_piece_repeats_first")
    pieces = cut(TEXTS["second_piece_repeats_first"])
    assert pieces[1][:1024] == pieces[0][-1024:]
    assert zlib.decompressobj(31).decompress(members[1]) == pieces[1]
    assert tokens[1][0] == pieces[1][0]                                             # the first token of a member is a literal


def test_nothing_to_match_gives_todays_member(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "no_trigram_repeat")
    assert (plain[0][18] & 7) == 0b101 and len(plain[0]) < len(TEXTS["no_trigram_repeat"])   # worth coding
    assert members == plain
    members, plain, tokens = run_case(hip_ctx, "random_70000")
    assert members == plain and all(m[18] == 0x01 for m in members)               # stored, as today


def test_matches_that_share_one_distance_symbol(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "one_distance_symbol")
    dist = {d for l, d in matches_of(tokens[0])}
    assert dist, "no match in a text that is one block twice"
    symbols = {max(i for i, b in enumerate(DIST_BASE) if b <= d) for d in dist}
    assert len(symbols) == 1
    assert len(members[0]) < len(plain[0])


def test_the_ring_under_15_bit_literals_and_a_far_repeat(hip_ctx):
    members, plain, tokens = run_case(hip_ctx, "fibonacci_far_repeat")
    lens, _ = P.literal_code_lengths(plain[0])
    assert max(lens) == 15                                                          # the case is what it claims


@pytest.mark.parametrize("name", ["fastq_200k", "binned_200k", "distances"])
def test_a_member_is_a_function_of_its_piece(hip_ctx, name):
    from colorid_amd.hip import bgzf_deflate
    members, _, _ = run_case(hip_ctx, name)
    alone = [bgzf_deflate(hip_ctx, p, matches=True)[0] for p in cut(TEXTS[name])]
    assert alone == members


def test_a_wave_takes_more_than_one_member(hip_ctx):
    """16 x CUs + 7 pieces alternating two contents: every wave takes a second and a third member, and the table of the one before
    must not leak into them — the blob is the per-piece calls' members in turn"""
    import torch
    from colorid_amd.hip import bgzf_deflate
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16 * n_cu + 7
    a, b = TEXTS["binned_200k"][:BLOCK], TEXTS["fastq_200k"][BLOCK:2 * BLOCK]
    tail = TEXTS["binned_200k"][BLOCK:BLOCK + 777]
    alone = [bgzf_deflate(hip_ctx, p, matches=True)[0] for p in (a, b, tail)]
    for m, p in zip(alone, (a, b, tail)):
        check_lz_member(m, p)
    k = (n - 1) // 2
    text = np.concatenate([np.tile(np.frombuffer(a + b, np.uint8), k), np.frombuffer(a * ((n - 1) % 2) + tail + b"\0" * 16, np.uint8)])
    text_bytes = len(text) - 16
    assert (text_bytes + BLOCK - 1) // BLOCK == n
    d_out, lens, total = deflate_dev(hip_ctx, hip_ctx.lib.cid_bgzf_deflate_lz_dev, text, text_bytes)
    assert lens.tolist() == [len(alone[i % 2]) for i in range(n - 1)] + [len(alone[2])]
    assert total == int(lens.sum())
    row = torch.from_numpy(np.frombuffer(alone[0] + alone[1], np.uint8).copy()).cuda()
    same = d_out[:k * row.numel()].view(k, row.numel()) == row
    wrong = (~same.all(dim=1)).nonzero().flatten().tolist()
    assert not wrong, f"pairs {wrong[:8]} differ from the members of their pieces compressed alone"
    rest = d_out[k * row.numel():total].cpu().numpy().tobytes()
    assert rest == alone[0] * ((n - 1) % 2) + alone[2]
    del d_out, same, row
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- the finder finds something

def test_a_run_and_a_repeated_record_shrink_to_a_quarter(hip_ctx):
    """guards against a finder that does nothing (zlib level 1: 303 and 763 bytes; matches of 16 bytes alone would get under a quarter)"""
    for name in ("run_65280", "record_x300"):
        members, plain, tokens = run_case(hip_ctx, name)
        print(f"{name}: {len(members[0])} bytes with matches, {len(plain[0])} without")
        assert 4 * len(members[0]) <= len(plain[0])


@pytest.mark.parametrize("name", ["fastq_200k", "binned_200k"])
def test_fastq_is_smaller_than_without_matches(hip_ctx, name):
    members, plain, tokens = run_case(hip_ctx, name)
    lz, huff = sum(map(len, members)), sum(map(len, plain))

    def level1(p):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(co.compress(p) + co.flush()) + 26

    z1 = sum(level1(p) for p in cut(TEXTS[name]))
    share = (huff - lz) / (huff - z1) if huff != z1 else float("nan")
    print(f"{name}: literals only {huff} bytes, with matches {lz}, zlib level 1 {z1}: {100 * share:.1f} % of zlib level 1's saving")
    assert lz < huff


# ---------------------------------------------------------------------------------------------------------------- arguments

def test_bad_arguments_are_refused(hip_ctx):
    import torch
    lib = hip_ctx.lib
    text = TEXTS["fastq_200k"][:70_000]
    cap = lib.cid_bgzf_deflate_bound(len(text))
    d_text = torch.from_numpy(np.frombuffer(b"\0" * 16 + text + b"\0" * 16, np.uint8).copy()).cuda()
    d_out = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert d_text.data_ptr() % 16 == 0
    nm = C.c_size_t(99)
    good = (hip_ctx.h, d_text.data_ptr() + 16, len(text), d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    for at, value, why in ((1, d_text.data_ptr() + 17, b"16-byte aligned"), (4, cap - 1, b"cid_bgzf_deflate_bound"), (0, None, b"null"), (1, None, b"null"),
                           (3, None, b"null"), (6, None, b"null"), (7, None, b"null")):
        args = list(good)
        args[at] = value
        assert lib.cid_bgzf_deflate_lz_dev(*args) == CID_ERR_INVALID and why in lib.cid_last_error(), (at, lib.cid_last_error())
    assert lib.cid_ctx_synchronize(hip_ctx.h) == 0
    assert bool((d_out == 0xA5).all()) and d_len.cpu().tolist() == [0x5A5A5A5A] * 3 and int(d_total.cpu()[0]) == 0x5A5A5A5A5A5A
    # the host form: null pointers, and a buffer that the members do not fit says how much they take
    host = np.frombuffer(TEXTS["random_70000"], np.uint8)
    out = np.zeros(70_000, np.uint8)
    ln = np.zeros(2, np.uint32)
    nb = C.c_size_t(0)
    assert lib.cid_bgzf_deflate_lz(hip_ctx.h, host.ctypes.data, len(host), out.ctypes.data, out.size, C.byref(nb), ln.ctypes.data, C.byref(nm)) == CID_ERR_INVALID
    assert nb.value == 70_000 + 62 and not out.any()
    assert lib.cid_bgzf_deflate_lz(hip_ctx.h, None, len(host), out.ctypes.data, out.size, C.byref(nb), ln.ctypes.data, C.byref(nm)) == CID_ERR_INVALID
    assert lib.cid_bgzf_deflate_lz(None, host.ctypes.data, len(host), out.ctypes.data, out.size, C.byref(nb), ln.ctypes.data, C.byref(nm)) == CID_ERR_INVALID
    assert lib.cid_bgzf_deflate_lz(hip_ctx.h, host.ctypes.data, len(host), out.ctypes.data, out.size, None, ln.ctypes.data, C.byref(nm)) == CID_ERR_INVALID
