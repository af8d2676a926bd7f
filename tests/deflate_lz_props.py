"""What a member written by cid_bgzf_deflate_lz must satisfy, checked from the member's bytes and its piece alone: a plain DEFLATE reader
(RFC 1951) that turns a member into its tokens — a literal is an int, a match a (length, distance) pair —, the rules the tokens must keep
(check_tokens), and a small encoder over the fixed Huffman codes that the CPU tests use to write members that break one rule each.  RFC
1951 / RFC 1952 / SAM specification 4.1 are the only references: nothing here restates how the kernel finds or chooses its matches."""
import struct
import zlib

import numpy as np

from deflate_props import BLOCK, CL_ORDER, bgzf_wrap, huffman_bits, int_bits, split_members

# RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
# RFC 1951 3.2.6
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30
WINDOW = 32768


class _Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data) + b"\0\0\0\0", 0
        self.end = 8 * len(data)

    def peek(self, n):
        b = self.pos >> 3
        return (int.from_bytes(self.d[b:b + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        assert self.pos + n <= self.end, "the stream runs past the member"
        v = self.peek(n)
        self.pos += n
        return v


def _decoder(lens):
    """code lengths -> (table indexed by the next `width` bits as they lie in the stream: (symbol, length) or None, width)"""
    width = max(lens) if len(lens) else 0
    assert width > 0, "a code without a symbol"
    table, code = [None] * (1 << width), 0
    for ln in range(1, width + 1):
        for sym, l in enumerate(lens):
            if l == ln:
                assert code < (1 << ln), "an over-subscribed code"
                rev = int(format(code, "0%db" % ln)[::-1], 2)                    # DEFLATE packs a code from its top bit
                for hi in range(1 << (width - ln)):
                    table[rev | (hi << ln)] = (sym, ln)
                code += 1
        code <<= 1
    return table, width


def _symbol(bits, dec):
    table, width = dec
    e = table[bits.peek(width)]
    assert e is not None, "bits that are no code"
    assert bits.pos + e[1] <= bits.end, "the stream runs past the member"
    bits.pos += e[1]
    return e[0]


def read_tokens(member):
    """one BGZF member -> (tokens, number of DEFLATE blocks, kinds of the blocks [0 stored | 1 fixed | 2 dynamic]); framing asserted"""
    assert member[:4] == b"\x1f\x8b\x08\x04", "gzip header with FEXTRA"
    assert struct.unpack_from("<H", member, 10)[0] == 6 and member[12:16] == b"BC\x02\x00", "the BC field"
    assert struct.unpack_from("<H", member, 16)[0] + 1 == len(member), "BSIZE + 1 is the member's length"
    body = member[18:-8]
    bits = _Bits(body)
    tokens, kinds = [], []
    while True:
        bfinal, btype = bits.take(1), bits.take(2)
        assert btype != 3, "block type 3"
        kinds.append(btype)
        if btype == 0:
            bits.pos = (bits.pos + 7) // 8 * 8
            n, nn = bits.take(16), bits.take(16)
            assert n ^ nn == 0xFFFF, "LEN / NLEN"
            at = bits.pos // 8
            assert at + n <= len(body), "the stored block runs past the member"
            tokens += list(body[at:at + n])
            bits.pos += 8 * n
        else:
            if btype == 1:
                lit, dist = _decoder(FIXED_LIT), _decoder(FIXED_DIST)
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                assert hlit <= 286 and hdist <= 30, "HLIT / HDIST"
                cl = [0] * 19
                for sym in CL_ORDER[:hclen]:
                    cl[sym] = bits.take(3)
                cld, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    sym = _symbol(bits, cld)
                    if sym < 16:
                        lens.append(sym)
                    elif sym == 16:
                        assert lens, "a repeat with nothing before it"
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * ((3 + bits.take(3)) if sym == 17 else (11 + bits.take(7)))
                assert len(lens) == hlit + hdist, "a run crosses the end of the declared lengths"
                assert lens[256], "no code for the end-of-block"
                lit = _decoder(lens[:hlit])
                dist = _decoder(lens[hlit:]) if any(lens[hlit:]) else None
            while True:
                sym = _symbol(bits, lit)
                if sym < 256:
                    tokens.append(sym)
                elif sym == 256:
                    break
                else:
                    assert sym <= 285, "length symbol 286 or 287"
                    length = LEN_BASE[sym - 257] + bits.take(LEN_EXTRA[sym - 257])
                    assert dist is not None, "a match without a distance code"
                    ds = _symbol(bits, dist)
                    assert ds < 30, "distance symbol 30 or 31"
                    tokens.append((length, DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])))
        if bfinal:
            break
    assert (bits.pos + 7) // 8 == len(body), "bytes between the last block and the trailer"
    return tokens, len(kinds), kinds


def check_tokens(tokens, piece):
    """every length 3 .. 258, every distance <= 32 768 and <= the bytes produced so far, and the tokens reproduce `piece`"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            length, distance = t
            assert 3 <= length <= 258, f"a match of length {length}"
            assert 1 <= distance <= WINDOW, f"a distance of {distance}"
            assert distance <= len(out), f"a distance of {distance} after {len(out)} bytes: the source lies before the member's first byte"
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
        else:
            assert 0 <= t <= 255
            out.append(t)
        assert len(out) <= len(piece), "more bytes than the piece has"
    assert bytes(out) == piece, "the tokens give another text"


def check_lz_member(member, piece):
    """Everything a member of cid_bgzf_deflate_lz must satisfy, from its bytes and its piece alone -> its tokens"""
    tokens, n_blocks, kinds = read_tokens(member)
    assert n_blocks == 1, "more than one block"
    crc, isize = struct.unpack("<II", member[-8:])
    assert crc == zlib.crc32(piece) & 0xFFFFFFFF, "CRC-32"
    assert isize == len(piece), "ISIZE"
    check_tokens(tokens, piece)
    d = zlib.decompressobj(31)
    try:
        got = d.decompress(member)
    except zlib.error as e:
        raise AssertionError(f"zlib refuses the member: {e}")
    assert d.eof and d.unused_data == b"" and got == piece, "zlib: another text, or the member and its stream end apart"
    return tokens


def check_lz_blob(blob, member_len, pieces):
    """check_lz_member over the members of a blob -> (members, [tokens])"""
    members = split_members(blob)
    assert [len(m) for m in members] == [int(x) for x in member_len] and len(members) == len(pieces)
    return members, [check_lz_member(m, p) for m, p in zip(members, pieces)]


def matches_of(tokens):
    return [t for t in tokens if isinstance(t, tuple)]


# ---------------------------------------------------------------------------------------------------------------- a fixed-code encoder

def _len_symbol(length):
    s = max(i for i, b in enumerate(LEN_BASE) if b <= length)
    return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]


def _dist_symbol(distance):
    s = max(i for i, b in enumerate(DIST_BASE) if b <= distance)
    return s, DIST_EXTRA[s], distance - DIST_BASE[s]


def encode_fixed(tokens, piece, blocks=1):
    """the tokens as one BGZF member of `blocks` fixed-Huffman blocks (the tokens dealt evenly); CRC-32 and ISIZE are `piece`'s.  Nothing
    is checked: this writes the broken members of the CPU tests as readily as good ones (distances must fit a distance symbol)."""
    parts, per = [], (len(tokens) + blocks - 1) // blocks
    for b in range(blocks):
        parts.append(int_bits((1 if b == blocks - 1 else 0) | (1 << 1), 3))
        for t in tokens[b * per:(b + 1) * per]:
            if isinstance(t, tuple):
                ls, leb, lex = _len_symbol(t[0])
                ds, deb, dex = _dist_symbol(t[1])
                parts += [huffman_bits([ls], FIXED_LIT), int_bits(lex, leb), huffman_bits([ds], FIXED_DIST), int_bits(dex, deb)]
            else:
                parts.append(huffman_bits([t], FIXED_LIT))
        parts.append(huffman_bits([256], FIXED_LIT))
    bits = np.concatenate(parts)
    bits = np.concatenate([bits, np.zeros(-len(bits) % 8, np.uint8)])
    return bgzf_wrap(np.packbits(bits, bitorder="little").tobytes(), piece)


# ---------------------------------------------------------------------------------------------------------------- texts

def binned_fastq(rng, n_bytes):
    """FASTQ with Illumina-style headers and binned qualities: 4 quality letters, mostly F (what recent instruments write)"""
    out, size, i = [], 0, 0
    letters = np.frombuffer(b"F:,#", np.uint8)
    while size < n_bytes:
        q = letters[rng.choice(4, size=150, p=[0.9, 0.06, 0.03, 0.01])]
        rec = (b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n" % (1101 + i // 5000, 1000 + (i * 37) % 30000, 1000 + (i * 101) % 30000) +
               bytes(rng.choice(list(b"ACGT"), size=150).astype(np.uint8)) + b"\n+\n" + q.tobytes() + b"\n")
        out.append(rec); size += len(rec); i += 1
    return b"".join(out)[:n_bytes]


def cut(text):
    return [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]
