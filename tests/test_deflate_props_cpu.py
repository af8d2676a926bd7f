"""tests/deflate_props.py before anything depends on it: check_member accepts members made by zlib (Huffman only) and by the plain host
encoder of the compressor's layout, and refuses every single broken property of an otherwise valid member; and the generated texts
are what they claim, by the plain Huffman tree over the text alone.  No GPU."""
import struct
import zlib

import numpy as np
import pytest

import deflate_props as P
from deflate_props import BLOCK, check_member, encode_member, piece_histogram, plain_huffman


def _fastq(n=30_000):
    return P.illumina_fastq(np.random.default_rng(5), n)


def zlib_member(piece):
    """zlib's Huffman-only stream (memLevel 9: one block up to 32 767 literals) as a BGZF member"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    return P.bgzf_wrap(co.compress(piece) + co.flush(), piece)


# ---------------------------------------------------------------------------------------------------------------- the checker

@pytest.mark.parametrize("name", ["fastq", "cl_limit_14", "cl_limit_13"])
def test_checker_accepts_zlib_members(name):
    piece = _fastq() if name == "fastq" else P.cl_limit_texts()[name]
    member = zlib_member(piece)
    assert member[18] & 7 == 0b101, "zlib wrote one final dynamic block"
    kind, lit, cl = check_member(member, piece, own=False)
    assert kind == "coded" and len(lit) == 257 and len(cl) == 19
    assert any(s >= 16 for s in P.parse_dynamic_header(member)["cl_syms"])       # zlib writes run codes: the parser reads them,
    with pytest.raises(AssertionError, match="run codes|HDIST"):                   # and they are no member of this compressor's
        check_member(member, piece)


def test_checker_accepts_the_host_encoder_and_stored_members():
    piece = _fastq()
    kind, lit, cl = check_member(encode_member(piece), piece)
    assert kind == "coded" and lit == plain_huffman(piece_histogram(piece))[2]
    assert cl == plain_huffman(P.code_length_histogram(lit + [1, 1]))[2]
    rnd = bytes(np.random.default_rng(6).integers(0, 256, 5000).astype(np.uint8))
    stored = P.bgzf_wrap(b"\x01" + struct.pack("<HH", len(rnd), len(rnd) ^ 0xFFFF) + rnd, rnd)
    assert check_member(stored, rnd) == ("stored", [], [])
    assert check_member(P.bgzf_wrap(b"\x01\x01\x00\xfe\xffA", b"A"), b"A")[0] == "stored"


def _swap_frequent_and_rare(piece):
    hist = piece_histogram(piece)
    _, _, lens = plain_huffman(hist)
    used = [s for s in range(256) if hist[s]]
    a, b = max(used, key=lambda s: hist[s]), min(used, key=lambda s: hist[s])
    assert lens[a] < lens[b]
    lens[a], lens[b] = lens[b], lens[a]
    return encode_member(piece, lens)


def _cl_entry_off_kraft(piece):
    _, _, lit = plain_huffman(piece_histogram(piece))
    _, _, cl = plain_huffman(P.code_length_histogram(lit + [1, 1]))
    cl[max(range(19), key=lambda s: cl[s])] -= 1                                 # a deepest leaf one level up: over-subscribed
    return encode_member(piece, lit, cl)


def _cl_frequent_and_rare_swapped(piece):
    _, _, lit = plain_huffman(piece_histogram(piece))
    freq = P.code_length_histogram(lit + [1, 1])
    _, _, cl = plain_huffman(freq)
    used = [s for s in range(19) if freq[s]]
    a, b = max(used, key=lambda s: freq[s]), min(used, key=lambda s: freq[s])
    cl[a], cl[b] = cl[b], cl[a]
    return encode_member(piece, lit, cl)


def _flat_literal_code(piece):
    """a complete code that keeps the order of the frequencies but is no Huffman code: only the cost tells"""
    hist = piece_histogram(piece)
    used = sorted((s for s in range(257) if hist[s]), key=lambda s: -hist[s])
    k = (len(used) - 1).bit_length()                                             # 2^k - u codes of k - 1 bits and 2u - 2^k of k bits: Kraft sum 1
    lens = [0] * 257
    for rank, s in enumerate(used):
        lens[s] = k - 1 if rank < (1 << k) - len(used) else k
    return encode_member(piece, lens)


def _flat_code_length_code(piece):
    """the same for the code-length code"""
    _, _, lit = plain_huffman(piece_histogram(piece))
    freq = P.code_length_histogram(lit + [1, 1])
    used = sorted((s for s in range(19) if freq[s]), key=lambda s: -freq[s])
    k = (len(used) - 1).bit_length()
    cl = [0] * 19
    for rank, s in enumerate(used):
        cl[s] = k - 1 if rank < (1 << k) - len(used) else k
    return encode_member(piece, lit, cl)


def _length_for_an_unused_value(piece):
    """the rarest literal's leaf split in two, the new leaf given to a byte value that does not occur: still a complete code"""
    hist = piece_histogram(piece)
    _, _, lens = plain_huffman(hist)
    rare = min((s for s in range(256) if hist[s]), key=lambda s: (-lens[s], hist[s]))
    unused = next(s for s in range(256) if not hist[s])
    lens[rare] += 1
    lens[unused] = lens[rare]
    return encode_member(piece, lens)


def _patch(member, at, value):
    m = bytearray(member)
    m[at] = value
    return bytes(m)


def _with_bsize(member, bsize):
    return member[:16] + struct.pack("<H", bsize) + member[18:]


def _padding_piece():
    """a FASTQ cut whose coded form leaves bits behind the end-of-block"""
    for n in range(30_000, 30_016):
        piece = _fastq(n)
        h = P.parse_dynamic_header(encode_member(piece))
        lit = h["lens"][:257]
        if (h["end"] + sum(f * l for f, l in zip(piece_histogram(piece), lit))) % 8:
            return piece
    raise AssertionError("no cut leaves padding bits")


CORRUPTIONS = {
    "frequent_and_rare_literal_lengths_swapped": (lambda p: _swap_frequent_and_rare(p), "longer code than a less frequent|costs"),
    "code_length_entry_off_the_kraft_sum": (lambda p: _cl_entry_off_kraft(p), "zlib refuses|Kraft"),
    "code_length_lengths_swapped": (lambda p: _cl_frequent_and_rare_swapped(p), "code lengths: a symbol has a longer code"),
    "literal_code_complete_but_not_huffman": (lambda p: _flat_literal_code(p), "the literal code costs"),
    "code_length_code_complete_but_not_huffman": (lambda p: _flat_code_length_code(p), "the code-length code costs"),
    "length_for_a_value_that_does_not_occur": (lambda p: _length_for_an_unused_value(p), "non-zero exactly for the byte values"),
    "nonzero_padding_bits": (lambda p: encode_member(p, pad_bits=0x7F), "non-zero bits behind the end-of-block"),
    "bsize_one_more": (lambda p: _with_bsize(encode_member(p), len(encode_member(p))), "BSIZE"),
    "bsize_one_less": (lambda p: _with_bsize(encode_member(p), len(encode_member(p)) - 2), "BSIZE"),
    "crc": (lambda p: _patch(encode_member(p), -5, encode_member(p)[-5] ^ 1), "zlib refuses|CRC"),
    "isize": (lambda p: _patch(encode_member(p), -4, encode_member(p)[-4] ^ 1), "zlib refuses|ISIZE"),
    "bc_field": (lambda p: _patch(encode_member(p), 12, ord("b")), "BC field"),
    "a_byte_behind_the_member": (lambda p: encode_member(p) + b"\0", "bytes behind the member"),
    "truncated": (lambda p: encode_member(p)[:-1], "ends before its stream"),
    "another_text": (lambda p: encode_member(p[:-1] + b"#"), "another text|zlib refuses"),
}


@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_checker_rejects_one_broken_property(name):
    piece = _padding_piece()
    check_member(encode_member(piece), piece)                                    # the member the corruption starts from is accepted
    make, message = CORRUPTIONS[name]
    with pytest.raises(AssertionError, match=message):
        check_member(make(piece), piece)


def test_checker_rejects_a_coded_member_as_long_as_the_stored_form():
    piece = P.break_even_piece()
    member = encode_member(piece)
    assert len(member) == len(piece) + 31
    with pytest.raises(AssertionError, match="coded although not shorter"):
        check_member(member, piece)
    stored = P.bgzf_wrap(b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece, piece)
    assert check_member(stored, piece)[0] == "stored"                              # and storing it is right
    # one byte more than the stored form: refused by the bound every member has
    longer = bytes(np.random.default_rng(8).integers(0, 256, 600).astype(np.uint8))
    with pytest.raises(AssertionError, match="longer than the stored form"):
        check_member(encode_member(longer), longer)


def test_checker_rejects_a_stored_member_of_a_piece_that_compresses_well():
    piece = _fastq()
    stored = P.bgzf_wrap(b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece, piece)
    with pytest.raises(AssertionError, match="stored although the coded form is smaller"):
        check_member(stored, piece)
    for at, msg in ((19, "LEN"), (21, "LEN")):                                   # zlib checks LEN against NLEN; both patched, the text changes
        with pytest.raises(AssertionError, match="zlib|LEN"):
            check_member(_patch(stored, at, stored[at] ^ 1), piece)
    with pytest.raises(AssertionError, match="more than one block|zlib"):
        check_member(_patch(stored, 18, 0), piece)


def test_checker_rejects_what_is_not_this_compressors_layout():
    piece = _fastq()
    # valid members (zlib reads them, and the checker does with own=False), but not this compressor's
    for kwargs, message in (({"dist_lens": (1,)}, "HDIST 2"), ({"dist_lens": (1, 0)}, "HDIST 2"), ({"dist_lens": (1, 1, 0)}, "HDIST 2")):
        member = encode_member(piece, **kwargs)
        assert check_member(member, piece, own=False)[0] == "coded"
        with pytest.raises(AssertionError, match=message):
            check_member(member, piece)
    for own in (True, False):
        with pytest.raises(AssertionError, match="HLIT"):
            check_member(encode_member(piece, extra_lit=1), piece, own)


# ---------------------------------------------------------------------------------------------------------------- the generators

@pytest.mark.parametrize("name", list(P.CL_LIMIT_TABLES))
def test_cl_limit_texts_force_a_code_length_tree_deeper_than_7(name):
    piece = P.cl_limit_texts()[name]
    lmax, design = P.cl_limit_design(name)
    hist = piece_histogram(piece)
    total = sum(hist)
    assert total == 1 << lmax and len(piece) == total - 1
    assert all(f & (f - 1) == 0 for f in hist if f)                               # dyadic: a symbol of count f has probability 2^-l,
    forced = [lmax - (f.bit_length() - 1) if f else 0 for f in hist]              # l = Lmax - log2 f, and a code of cost = entropy has no other lengths
    cost, depth, lens = plain_huffman(hist)
    assert lens == forced and sorted(l for l in lens if l) == sorted(design) and depth == lmax <= 15
    assert cost == sum(f * l for f, l in zip(hist, forced))
    cl_cost, cl_depth, _ = plain_huffman(P.code_length_histogram(forced + [1, 1]))
    print(f"{name}: {len(piece)} bytes, {sum(1 for f in hist if f)} symbols, the code-length tree is {cl_depth} deep")
    assert cl_depth > 7
    assert P.unlimited_huffman_depth(piece) == lmax


@pytest.mark.parametrize("name", list(P.CLUSTER_ROUNDS))
def test_clustered_texts_fill_the_ring_in_the_round_they_claim(name):
    piece = P.clustered_texts()[name]
    _, depth, lens = plain_huffman(piece_histogram(piece))
    assert depth <= 15
    words = P.round_words(piece, lens)
    dense = int(np.argmax(words))
    print(f"{name}: {len(piece)} bytes, round {dense} of {len(words)} takes {words[dense]:.1f} words, the next {sorted(words)[-2]:.1f}")
    assert dense == P.CLUSTER_ROUNDS[name]
    assert 400 < words[dense] <= 480
    if name == "cluster_last":
        assert len(piece) % 1024 and dense == len(words) - 1
    else:
        assert len(piece) == BLOCK
    # a member of the host encoder over it passes the checker (15-bit leaves, all 256 values)
    assert check_member(encode_member(piece), piece)[0] == "coded"


def test_short_texts_cover_the_lengths_and_alphabets():
    texts = P.short_texts()
    for n in P.SHORT_LENGTHS:
        assert len(texts[f"two_letter_{n}"]) == n == len(texts[f"fastq_{n}"])
        assert set(texts[f"two_letter_{n}"]) <= set(b"AC")
    assert {1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025} <= set(P.SHORT_LENGTHS)
    assert [len(set(texts[f"two_symbols_{n}"])) for n in (2, 3, 5)] == [2, 2, 2]
    assert texts == P.short_texts()                                              # seeded


def test_alignment_and_stride_texts_have_the_shapes_they_claim():
    for name, text in P.alignment_texts().items():
        n = (len(text) + BLOCK - 1) // BLOCK
        assert 5 <= n <= 8 and str(n) in name and len(text) % BLOCK
    period, tail = P.stride_pieces()
    text = P.stride_text(8)
    assert len(text) == 7 * BLOCK + len(tail) and 0 < len(tail) < BLOCK
    for i in range(7):
        assert text[i * BLOCK:(i + 1) * BLOCK].tobytes() == period[i % 3]
    assert text[7 * BLOCK:].tobytes() == tail
