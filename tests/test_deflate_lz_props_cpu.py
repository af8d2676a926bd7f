"""tests/deflate_lz_props.py proven on the CPU: the DEFLATE reader and check_lz_member accept what zlib writes and what today's compressor
writes, and refuse members that break one rule each."""
import struct
import zlib

import numpy as np
import pytest

import deflate_props as P
from deflate_lz_props import (DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, binned_fastq, check_lz_member, check_tokens, encode_fixed, matches_of,
                              read_tokens)


def raw_deflate(piece, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(piece) + co.flush()


@pytest.fixture(scope="module")
def fastq():
    return binned_fastq(np.random.default_rng(11), 20_000)


def test_the_tables_are_rfc_1951s():
    assert len(LEN_BASE) == len(LEN_EXTRA) == 29 and len(DIST_BASE) == len(DIST_EXTRA) == 30
    for base, extra in ((LEN_BASE[:-1], LEN_EXTRA[:-1]), (DIST_BASE, DIST_EXTRA)):   # every range begins where the one before ends
        assert all(base[i] + (1 << extra[i]) == base[i + 1] for i in range(len(base) - 1))
    assert LEN_BASE[27] + (1 << LEN_EXTRA[27]) - 1 == 258 and (LEN_BASE[28], LEN_EXTRA[28]) == (258, 0)   # 258: symbol 285, no extra bits
    assert DIST_BASE[29] + (1 << DIST_EXTRA[29]) - 1 == 32768


@pytest.mark.parametrize("level", [1, 6])
def test_accepts_zlib_streams(fastq, level):
    member = P.bgzf_wrap(raw_deflate(fastq, level), fastq)
    tokens = check_lz_member(member, fastq)
    assert matches_of(tokens), "zlib found no match in FASTQ"
    assert read_tokens(member)[2] == [2]


def test_accepts_a_fixed_block_and_short_texts():
    for piece in (b"a", b"ab", b"abcabcabcabcabc", b"G" * 700):
        member = P.bgzf_wrap(raw_deflate(piece, 6, zlib.Z_FIXED), piece)
        check_lz_member(member, piece)
        assert read_tokens(member)[2] == [1]
    tokens = check_lz_member(P.bgzf_wrap(raw_deflate(b"G" * 700, 6, zlib.Z_FIXED), b"G" * 700), b"G" * 700)
    assert (258, 1) in tokens                                                       # an overlapping copy of the longest length


def test_accepts_todays_host_encoded_members(fastq):
    for piece in (fastq, P.short_texts()["two_letter_4097"]):
        tokens = check_lz_member(P.encode_member(piece), piece)
        assert tokens == list(piece)
    piece = bytes(np.random.default_rng(5).integers(0, 256, 3000).astype(np.uint8))
    stored = P.bgzf_wrap(b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece, piece)
    assert check_lz_member(stored, piece) == list(piece)


def test_the_encoder_and_the_reader_agree():
    piece = b"abcdefgh" * 40 + b"xyz" + b"abcdefgh" * 3
    tokens = list(piece[:8]) + [(258, 8), (54, 8)] + list(b"xyz") + [(8, 11), (16, 8)]
    member = encode_fixed(tokens, piece)
    assert check_lz_member(member, piece) == tokens


def test_rejects_a_distance_beyond_the_start():
    piece = b"abcabc"
    good = encode_fixed(list(b"abc") + [(3, 3)], piece)
    check_lz_member(good, piece)
    bad = encode_fixed(list(b"abc") + [(3, 4)], piece)                              # one byte before the member's first
    with pytest.raises(AssertionError, match="before the member's first byte"):
        check_lz_member(bad, piece)
    first = encode_fixed([(3, 1)] + list(b"abc"), piece)                            # a match as the first token
    with pytest.raises(AssertionError, match="before the member's first byte"):
        check_lz_member(first, piece)


def test_rejects_a_distance_of_32769():
    """no distance symbol reaches 32 769 (symbol 29 ends at 32 768), so the rule is put to the tokens themselves"""
    rng = np.random.default_rng(9)
    head = bytes(rng.integers(0, 256, 32769).astype(np.uint8))
    check_tokens(list(head) + [(4, 32768)], head + head[1:5])
    with pytest.raises(AssertionError, match="a distance of 32769"):
        check_tokens(list(head) + [(4, 32769)], head + head[0:4])
    with pytest.raises(AssertionError, match="length"):
        check_tokens(list(b"aaaa") + [(2, 1)], b"aaaaaa")
    with pytest.raises(AssertionError, match="length"):
        check_tokens(list(b"a") + [(259, 1)], b"a" * 260)


def test_rejects_a_second_block(fastq):
    two = encode_fixed(list(fastq[:100]), fastq[:100], blocks=2)
    assert zlib.decompressobj(31).decompress(two) == fastq[:100]                    # a good gzip member, but not one block
    with pytest.raises(AssertionError, match="more than one block"):
        check_lz_member(two, fastq[:100])
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(fastq[:9000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(fastq[9000:]) + co.flush()
    with pytest.raises(AssertionError, match="more than one block"):
        check_lz_member(P.bgzf_wrap(body, fastq), fastq)


def test_rejects_a_wrong_crc_isize_bsize_and_text(fastq):
    member = P.bgzf_wrap(raw_deflate(fastq, 1), fastq)
    check_lz_member(member, fastq)
    crc = bytearray(member); crc[-5] ^= 0x10
    with pytest.raises(AssertionError, match="CRC-32"):
        check_lz_member(bytes(crc), fastq)
    isize = bytearray(member); isize[-4] ^= 1
    with pytest.raises(AssertionError, match="ISIZE"):
        check_lz_member(bytes(isize), fastq)
    with pytest.raises(AssertionError, match="BSIZE"):
        check_lz_member(member + b"\0", fastq)
    other = fastq[:-1] + b"#"
    wrong = P.bgzf_wrap(raw_deflate(fastq, 1), other)                               # the trailer of another text
    with pytest.raises(AssertionError, match="another text"):
        check_lz_member(wrong, other)
