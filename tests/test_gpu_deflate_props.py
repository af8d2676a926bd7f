"""cid_bgzf_deflate on the paths its first table of texts left alone (tests/deflate_props.py has the texts and the checker): the 7-bit
limit of the code-length code, the output ring at its stated bound, one wave taking more than one member, short pieces, the gather's
four destination alignments, the quality of the codes, and the alignment refusal.  Every case: check_member per member, a second call
gives the same bytes, and cid_bgzf_inflate reads the members back."""
import ctypes as C
import time

import numpy as np
import pytest

import deflate_props as P
from colorid_amd._lib import CID_ERR_INVALID
from deflate_props import BLOCK, check_blob, check_member, plain_huffman
from test_gpu_inflate import inflate

pytestmark = pytest.mark.gpu


def cut(text):
    return [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]


def cl_tree_depth(lit):
    """the depth of the plain tree over the histogram of a member's own 259 declared lengths"""
    return plain_huffman(P.code_length_histogram(list(lit) + [1, 1]))[1]


def run_case(ctx, text, read_back=True):
    """text -> (members, [(kind, literal lengths, code-length lengths)], member_len): checked, deterministic, read back by the device"""
    from colorid_amd.hip import bgzf_deflate
    blob, member_len = bgzf_deflate(ctx, text)
    pieces = cut(text)
    members, results = check_blob(blob, member_len, pieces)
    assert len(blob) <= ctx.lib.cid_bgzf_deflate_bound(len(text))
    blob2, member_len2 = bgzf_deflate(ctx, text)
    assert blob2 == blob and member_len2.tolist() == member_len.tolist(), "a second call gives other bytes"
    if read_back:
        read_back_members(ctx, members, pieces)
    return members, results, member_len


def read_back_members(ctx, members, pieces):
    rc, out, bad, _ = inflate(ctx.lib, ctx, members, [len(p) for p in pieces])
    assert rc == 0, ctx.lib.cid_last_error()
    assert out == b"".join(pieces)


def deflate_dev(ctx, text_array, text_bytes):
    """cid_bgzf_deflate_dev over a host uint8 array that ends in 16 bytes of padding -> (d_out, member lengths [numpy], total)"""
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
    rc = lib.cid_bgzf_deflate_dev(ctx.h, d_text.data_ptr(), text_bytes, d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    assert rc == 0, lib.cid_last_error()
    assert lib.cid_ctx_synchronize(ctx.h) == 0
    assert nm.value == n
    del d_text
    return d_out, d_len.cpu().numpy()[:n].astype(np.int64), int(d_total.cpu()[0])


def summary(group, results, depths):
    kinds = [r[0] for r in results]
    print(f"{group}: {kinds.count('coded')} coded, {kinds.count('stored')} stored; deepest unlimited code-length tree {max(depths) if depths else 0}")


@pytest.mark.parametrize("name", list(P.CL_LIMIT_TABLES))
def test_code_length_code_at_its_7_bit_limit(hip_ctx, name):
    text = P.cl_limit_texts()[name]
    members, results, _ = run_case(hip_ctx, text)
    kind, lit, cl = results[0]
    assert kind == "coded"
    depth = cl_tree_depth(lit)
    summary(name, results, [depth])
    assert depth > 7                                                             # the case is what it claims on the device's own lengths,
    assert max(cl) == 7                                                          # and the limited code reaches the limit


@pytest.mark.parametrize("name", list(P.CLUSTER_ROUNDS))
def test_output_ring_at_its_bound(hip_ctx, name):
    text = P.clustered_texts()[name]
    members, results, _ = run_case(hip_ctx, text)
    kind, lit, cl = results[0]
    assert kind == "coded"
    words = P.round_words(text, lit)
    dense = int(np.argmax(words))
    summary(name, results, [cl_tree_depth(lit)])
    print(f"{name}: round {dense} of {len(words)} takes {words[dense]:.1f} of the ring's 512 words")
    assert dense == P.CLUSTER_ROUNDS[name] and 400 < words[dense] <= 480


def test_short_pieces(hip_ctx):
    texts = P.short_texts()
    texts["break_even"] = P.break_even_piece()
    all_members, all_pieces, results, depths, coded_lengths = [], [], [], [], []
    for name, text in texts.items():
        members, res, member_len = run_case(hip_ctx, text, read_back=False)
        assert len(members) == 1
        all_members += members; all_pieces.append(text); results += res
        if res[0][0] == "coded":
            coded_lengths.append((len(text), name))
            depths.append(cl_tree_depth(res[0][1]))
        # the device form, byte for byte
        d_out, lens, total = deflate_dev(hip_ctx, np.frombuffer(text + b"\0" * 16, np.uint8).copy(), len(text))
        assert total == len(members[0]) and lens.tolist() == [total], name
        assert d_out.cpu().numpy()[:total].tobytes() == members[0], name
    read_back_members(hip_ctx, all_members, all_pieces)
    summary("short", results, depths)
    kinds = {r[0] for r in results}
    assert kinds == {"coded", "stored"}
    print(f"short: the shortest coded piece is {min(coded_lengths)[1]} ({min(coded_lengths)[0]} bytes); stored up to {max(len(p) for p, r in zip(all_pieces, results) if r[0] == 'stored')} bytes")
    # one literal and the end-of-block or two literals: the 259 lengths alone take 33 bytes, so the shortest pieces are stored
    assert results[list(texts).index("two_letter_1")][0] == "stored"
    assert results[list(texts).index("break_even")][0] == "stored"              # coded would be as long: "stored when that is not smaller"
    assert results[list(texts).index("two_letter_4097")][0] == "coded" and results[list(texts).index("fastq_4097")][0] == "coded"


def test_gather_at_every_destination_alignment(hip_ctx):
    from colorid_amd.hip import bgzf_deflate
    residues, results, depths = set(), [], []
    for name, text in P.alignment_texts().items():
        members, res, member_len = run_case(hip_ctx, text)
        assert 5 <= len(members) <= 8
        off = np.cumsum(member_len.astype(np.int64))[:-1]                        # where the members after the first begin
        residues |= {int(o) % 4 for o in off}
        print(f"{name}: members begin at {[0] + off.tolist()} -> modulo 4 {[0] + (off % 4).tolist()}")
        # a member is a function of its piece alone: the blob is every piece compressed in a call of its own, back to back
        alone = [bgzf_deflate(hip_ctx, p)[0] for p in cut(text)]
        assert b"".join(members) == b"".join(alone)
        results += res
        depths += [cl_tree_depth(r[1]) for r in res if r[0] == "coded"]
    summary("alignment", results, depths)
    assert residues == {0, 1, 2, 3}
    assert {r[0] for r in results} == {"coded", "stored"}


def test_a_wave_takes_more_than_one_member(hip_ctx):
    """16 waves per CU are launched, so with 16 x CUs + 7 members seven waves take a second member: a stored one after a coded one, a
    coded one after a stored one, and the short tail after a whole piece."""
    import torch
    from colorid_amd.hip import bgzf_deflate
    t0 = time.perf_counter()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16 * n_cu + 7
    period, tail = P.stride_pieces()
    alone = [bgzf_deflate(hip_ctx, p)[0] for p in period + [tail]]
    text = P.stride_text(n, pad=16)
    text_bytes = len(text) - 16
    assert (text_bytes + BLOCK - 1) // BLOCK == n
    t1 = time.perf_counter()
    d_out, lens, total = deflate_dev(hip_ctx, text, text_bytes)
    t2 = time.perf_counter()
    want_lens = np.array([len(alone[i % 3]) for i in range(n - 1)] + [len(alone[3])], np.int64)
    assert lens.tolist() == want_lens.tolist()
    assert total == int(lens.sum())
    # member i is the single-call member of piece i % 3: whole periods compared on the device, the rest and the tail on the host
    row = torch.from_numpy(np.frombuffer(b"".join(alone[:3]), np.uint8).copy()).cuda()
    k = (n - 1) // 3
    same = d_out[:k * row.numel()].view(k, row.numel()) == row
    wrong = (~same.all(dim=1)).nonzero().flatten().tolist()
    assert not wrong, f"periods {wrong[:8]} differ from the members of their pieces compressed alone"
    rest = d_out[k * row.numel():total].cpu().numpy().tobytes()
    assert rest == b"".join(alone[i % 3] for i in range(3 * k, n - 1)) + alone[3]
    off = np.concatenate([[0], np.cumsum(lens)])
    results = []
    for i in [0, 1, 2, 16 * n_cu - 1, 16 * n_cu, 16 * n_cu + 1, n - 1]:
        member = d_out[int(off[i]):int(off[i + 1])].cpu().numpy().tobytes()
        piece = period[i % 3] if i < n - 1 else tail
        results.append(check_member(member, piece))
        read_back_members(hip_ctx, [member], [piece])
    kinds = [alone[i][18] & 7 for i in range(3)]
    assert kinds == [0b101, 0b001, 0b101]                                        # coded, stored, coded: both changes of kind occur in a wave
    n_stored = (n - 1 + 1) // 3
    summary("stride (the 7 members checked)", results, [cl_tree_depth(r[1]) for r in results if r[0] == "coded"])
    del d_out, same, row
    torch.cuda.empty_cache()
    print(f"stride: {n} members ({n_cu} CUs), {text_bytes} bytes -> {total}; {n - n_stored - (results[-1][0] == 'stored')} coded, "
          f"{n_stored + (results[-1][0] == 'stored')} stored; texts {t1 - t0:.2f} s, deflate with upload {t2 - t1:.2f} s, wall {time.perf_counter() - t0:.2f} s")


def test_unaligned_text_is_refused_and_nothing_written(hip_ctx):
    import torch
    lib = hip_ctx.lib
    text = P.illumina_fastq(np.random.default_rng(3), 70_000)
    cap = lib.cid_bgzf_deflate_bound(len(text))
    d_text = torch.from_numpy(np.frombuffer(b"\0" + text + b"\0" * 16, np.uint8).copy()).cuda()
    d_out = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert d_text.data_ptr() % 16 == 0
    nm = C.c_size_t(99)
    rc = lib.cid_bgzf_deflate_dev(hip_ctx.h, d_text.data_ptr() + 1, len(text), d_out.data_ptr(), cap, d_total.data_ptr(), d_len.data_ptr(), C.byref(nm))
    assert rc == CID_ERR_INVALID and b"16-byte aligned" in lib.cid_last_error()
    assert lib.cid_ctx_synchronize(hip_ctx.h) == 0
    assert bool((d_out == 0xA5).all()) and d_len.cpu().tolist() == [0x5A5A5A5A] * 3 and int(d_total.cpu()[0]) == 0x5A5A5A5A5A5A
