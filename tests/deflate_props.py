"""What a member written by cid_bgzf_deflate must satisfy, checked from the member's bytes and its piece alone (check_member), the seeded
texts that reach the compressor's less-travelled paths, and a plain host encoder of the same member layout (one dynamic block of
literals, HLIT 257, HDIST 2, no run codes) that the CPU tests use to prove the checker.  RFC 1951 / RFC 1952 / SAM specification 4.1
are the only references: nothing here restates how the kernel breaks ties."""
import heapq
import struct
import zlib

import numpy as np

BLOCK = 65280
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
MAX_HEADER_BITS = 17 + 3 * 19 + 259 * 7          # the largest block header this compressor can write


# ---------------------------------------------------------------------------------------------------------------- plain Huffman

def plain_huffman(freqs):
    """the plain (unlimited) Huffman tree over the non-zero entries of `freqs` -> (cost = sum of freq x length, depth, lengths [one per
    entry, 0 where freq is 0]); every Huffman tree over one histogram has the same cost, whichever way ties fall"""
    used = [i for i, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if len(used) < 2:
        for i in used:
            lens[i] = 1
        return sum(freqs[i] for i in used), len(used), lens
    parent = {}
    heap = [(int(freqs[i]), 0, i) for i in used]
    heapq.heapify(heap)
    nxt, cost = len(freqs), 0
    while len(heap) > 1:
        (a, da, ia), (b, db, ib) = heapq.heappop(heap), heapq.heappop(heap)
        parent[ia] = parent[ib] = nxt
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1, nxt))
        nxt += 1
    for i in used:
        d, node = 0, i
        while node in parent:
            node = parent[node]
            d += 1
        lens[i] = d
    return cost, heap[0][1], lens


def piece_histogram(piece):
    """counts of the 256 literals and the end-of-block"""
    return np.bincount(np.frombuffer(piece, np.uint8), minlength=256).tolist() + [1]


def unlimited_huffman_depth(piece):
    """the deepest leaf of the plain Huffman tree over a piece's literals and the end-of-block"""
    heap = [(c, 0) for c in np.bincount(np.frombuffer(piece, np.uint8), minlength=256).tolist() + [1] if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def code_length_histogram(lens):
    """how often each of the code lengths 0..15 is declared, one code-length symbol per length (no run codes)"""
    return np.bincount(np.asarray(lens, np.int64), minlength=19).tolist()


def round_words(piece, lit_lens):
    """the 32-bit words every aligned 1 KiB round of the piece takes under the literal lengths given"""
    bits = np.asarray(lit_lens, np.int64)[np.frombuffer(piece, np.uint8)]
    return [float(bits[r:r + 1024].sum()) / 32 for r in range(0, len(piece), 1024)]


# ---------------------------------------------------------------------------------------------------------------- the parser

def canonical_codes(lens):
    """RFC 1951 3.2.2: the codes of the symbols with a non-zero length, shorter first, symbols of one length in symbol order"""
    codes, code = [0] * len(lens), 0
    for ln in range(1, max(lens) + 1 if len(lens) else 1):
        for sym, l in enumerate(lens):
            if l == ln:
                codes[sym] = code
                code += 1
        code <<= 1
    return codes


def parse_dynamic_header(member):
    """the header of a member's first DEFLATE block when it is a dynamic-Huffman one (RFC 1951 3.2.7) -> dict: bfinal, btype, and for
    btype 2 hlit, hdist, hclen, cl (the 19 code-length code lengths), lens (the hlit + hdist declared lengths), cl_syms (the code-length
    symbols as written, 16-18 included), end (the bit of member[18:] behind the header)"""
    bits = np.unpackbits(np.frombuffer(member[18:], np.uint8), bitorder="little")
    pos = 0

    def take(n):
        nonlocal pos
        assert pos + n <= len(bits), "the header runs past the member"
        v = int(sum(int(b) << i for i, b in enumerate(bits[pos:pos + n])))
        pos += n
        return v

    h = {"bfinal": take(1), "btype": take(2)}
    if h["btype"] != 2:
        return h
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for sym in CL_ORDER[:hclen]:
        cl[sym] = take(3)
    codes, code = {}, 0                                                          # canonical: (length, code) -> symbol
    for ln in range(1, 8):
        for sym in range(19):
            if cl[sym] == ln:
                codes[(ln, code)] = sym
                code += 1
        code <<= 1
    out, syms = [], []
    while len(out) < hlit + hdist:
        ln, code = 0, 0
        while (ln, code) not in codes or ln == 0:
            assert ln < 7, "no code-length code matches"
            code = (code << 1) | take(1)
            ln += 1
        sym = codes[(ln, code)]
        syms.append(sym)
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            assert out, "a repeat with nothing before it"
            out += [out[-1]] * (3 + take(2))
        else:
            out += [0] * ((3 + take(3)) if sym == 17 else (11 + take(7)))
    assert len(out) == hlit + hdist, "a run crosses the end of the declared lengths"
    h.update(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, lens=out, cl_syms=syms, end=pos)
    return h


def literal_code_lengths(member):
    """(the literal/length code lengths, the 19 code-length code lengths) a dynamic-Huffman member declares (RFC 1951 3.2.7)"""
    h = parse_dynamic_header(member)
    assert (h["bfinal"], h["btype"]) == (1, 2)
    return h["lens"][:h["hlit"]], h["cl"]


def split_members(blob):
    """the members of a BGZF byte string by their BSIZE; every one must carry the "BC" field"""
    out, pos = [], 0
    while pos < len(blob):
        assert blob[pos:pos + 4] == b"\x1f\x8b\x08\x04", "gzip header with FEXTRA"
        xlen = struct.unpack_from("<H", blob, pos + 10)[0]
        assert xlen == 6 and blob[pos + 12:pos + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", blob, pos + 16)[0]
        out.append(blob[pos:pos + bsize + 1])
        pos += bsize + 1
    assert pos == len(blob)
    return out


def gunzip_members(blob):
    """zlib over one member after the other: Huffman codes, CRC-32 and ISIZE checked by zlib"""
    out, rest = [], blob
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return out


# ---------------------------------------------------------------------------------------------------------------- bits of a code

def huffman_bits(symbols, lens):
    """the symbols under the canonical code of `lens` as DEFLATE packs them (a code from its top bit), one array entry per bit"""
    lens_a, codes = np.asarray(lens, np.int64), np.asarray(canonical_codes(list(lens)), np.int64)
    sym = np.asarray(symbols, np.int64)
    L, code = lens_a[sym], codes[sym]
    assert (L > 0).all(), "a symbol without a code"
    start = np.cumsum(L) - L
    out = np.zeros(int(L.sum()), np.uint8)
    for k in range(int(L.max()) if len(L) else 0):
        m = L > k
        out[start[m] + k] = (code[m] >> (L[m] - 1 - k)) & 1
    return out


def int_bits(value, n):
    return np.array([(value >> i) & 1 for i in range(n)], np.uint8)


def bgzf_wrap(body, piece):
    """a DEFLATE stream as a BGZF member: gzip header with the "BC" field, CRC-32, ISIZE"""
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 18 + len(body) + 8 - 1) + body +
            struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))


def encode_member(piece, lit_lens=None, cl_lens=None, pad_bits=0, dist_lens=(1, 1), extra_lit=0):
    """a host encoder of the compressor's member layout: one final dynamic block, HLIT 257, HDIST 2 with both distance lengths 1, the 259
    lengths written one code-length symbol each, the literals, the end-of-block.  Lengths default to the plain Huffman ones (which must
    then fit 15 and 7 bits); `pad_bits` goes into the bits behind the end-of-block.  `dist_lens` and `extra_lit` (unused length codes
    declared behind the end-of-block) leave the layout on purpose."""
    if lit_lens is None:
        _, depth, lit_lens = plain_huffman(piece_histogram(piece))
        assert depth <= 15
    lens = list(lit_lens) + [0] * extra_lit + list(dist_lens)
    if cl_lens is None:
        _, depth, cl_lens = plain_huffman(code_length_histogram(lens))
        assert depth <= 7
    ncl = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
    parts = [int_bits(1 | (2 << 1) | (extra_lit << 3) | ((len(dist_lens) - 1) << 8) | ((ncl - 4) << 13), 17)]
    parts += [int_bits(cl_lens[s], 3) for s in CL_ORDER[:ncl]]
    parts.append(huffman_bits(lens, cl_lens))
    parts.append(huffman_bits(np.concatenate([np.frombuffer(piece, np.uint8).astype(np.int64), [256]]), lit_lens))
    bits = np.concatenate(parts)
    fill = -len(bits) % 8
    bits = np.concatenate([bits, int_bits(pad_bits, fill)])
    return bgzf_wrap(np.packbits(bits, bitorder="little").tobytes(), piece)


# ---------------------------------------------------------------------------------------------------------------- the checker

def _kraft(lens, maxbits):
    return sum(1 << (maxbits - l) for l in lens if l)


def _monotone(freqs, lens, what):
    f, l = np.asarray(freqs, np.int64), np.asarray(lens, np.int64)
    used = f > 0
    f, l = f[used], l[used]
    bad = (f[:, None] > f[None, :]) & (l[:, None] > l[None, :])
    assert not bad.any(), f"{what}: a symbol has a longer code than a less frequent one"


def check_member(member, piece, own=True):
    """Everything a member of cid_bgzf_deflate must satisfy, from its bytes and its piece alone -> (kind "coded" | "stored", the literal
    code lengths, the code-length code lengths) (two empty lists for a stored member).  `own=False` drops the two conditions that are
    this compressor's own choice and no property of a good member: HDIST 2 with two one-bit distance codes, and no run codes (16-18)
    among the declared lengths."""
    n = len(piece)
    # zlib returns the piece and ends exactly at the member's end
    d = zlib.decompressobj(31)
    try:
        got = d.decompress(member)
    except zlib.error as e:
        raise AssertionError(f"zlib refuses the member: {e}")
    assert d.eof, "zlib: the member ends before its stream does"
    assert d.unused_data == b"", "zlib: bytes behind the member's end"
    assert got == piece, "zlib: another text"
    # framing
    assert member[:4] == b"\x1f\x8b\x08\x04", "gzip header with FEXTRA"
    assert struct.unpack_from("<H", member, 10)[0] == 6 and member[12:16] == b"BC\x02\x00", "the BC field"
    assert struct.unpack_from("<H", member, 16)[0] == len(member) - 1, "BSIZE"
    crc, isize = struct.unpack("<II", member[-8:])
    assert crc == zlib.crc32(piece) & 0xFFFFFFFF, "CRC-32"
    assert isize == n, "ISIZE"
    assert len(member) <= n + 31, "longer than the stored form"
    hist = piece_histogram(piece)
    h_cost, h_depth, _ = plain_huffman(hist)
    h = parse_dynamic_header(member)
    assert h["bfinal"] == 1, "more than one block"
    assert h["btype"] in (0, 2), "neither stored nor dynamic"
    if h["btype"] == 0:
        assert member[18] == 0x01, "the stored block's first byte"
        assert struct.unpack_from("<HH", member, 19) == (n, n ^ 0xFFFF), "LEN / NLEN"
        assert len(member) == n + 31 and member[23:23 + n] == piece
        if h_depth <= 15:   # storing was not plainly wrong: even under the largest header the coded form would not have been smaller
            assert 18 + (MAX_HEADER_BITS + h_cost + 7) // 8 + 8 >= n + 31, "stored although the coded form is smaller"
        return "stored", [], []
    hlit, hdist, cl, lens = h["hlit"], h["hdist"], h["cl"], h["lens"]
    lit = lens[:hlit]
    assert hlit == 257, "HLIT"
    if own:
        assert hdist == 2 and lens[hlit:] == [1, 1], "HDIST 2, both distance lengths 1"
        assert all(s < 16 for s in h["cl_syms"]) and len(h["cl_syms"]) == 259, "run codes among the declared lengths"
    assert max(cl) <= 7 and _kraft(cl, 7) == 1 << 7, "the code-length code: longer than 7 bits or Kraft sum not 1"
    assert max(lit) <= 15 and _kraft(lit, 15) == 1 << 15, "the literal code: longer than 15 bits or Kraft sum not 1"
    assert [l != 0 for l in lit] == [f != 0 for f in hist], "a length is non-zero exactly for the byte values that occur, and 256"
    _monotone(hist, lit, "literals")
    cl_freq = np.bincount(np.asarray(h["cl_syms"], np.int64), minlength=19).tolist()
    assert [l != 0 for l in cl] == [f != 0 for f in cl_freq], "a code-length code length is non-zero exactly for the symbols written"
    _monotone(cl_freq, cl, "code lengths")
    # the literals and the end-of-block under the declared code, bit for bit; zeros up to the byte boundary; then the trailer
    bits = np.unpackbits(np.frombuffer(member[18:-8], np.uint8), bitorder="little")
    want = huffman_bits(np.concatenate([np.frombuffer(piece, np.uint8).astype(np.int64), [256]]), lit)
    end = h["end"] + len(want)
    assert (end + 7) // 8 * 8 == len(bits), "the stream is not the literals and one end-of-block"
    assert np.array_equal(bits[h["end"]:end], want), "the stream is not the literals and one end-of-block"
    assert not bits[end:].any(), "non-zero bits behind the end-of-block"
    assert len(member) < n + 31, "coded although not shorter than the stored form"
    # exact cost
    cost = sum(f * l for f, l in zip(hist, lit))
    if h_depth <= 15:
        assert cost == h_cost, f"the literal code costs {cost} bits, a Huffman code {h_cost}"
    else:
        assert cost >= h_cost
    c_cost, c_depth, _ = plain_huffman(cl_freq)
    cost = sum(f * l for f, l in zip(cl_freq, cl))
    if c_depth <= 7:
        assert cost == c_cost, f"the code-length code costs {cost} bits, a Huffman code {c_cost}"
    else:
        assert cost >= c_cost
    return "coded", lit, cl


def check_blob(blob, member_len, pieces, own=True):
    """check_member over the members of a blob -> [(kind, literal lengths, code-length lengths)]"""
    members = split_members(blob)
    assert [len(m) for m in members] == [int(x) for x in member_len] and len(members) == len(pieces)
    return members, [check_member(m, p, own) for m, p in zip(members, pieces)]


# ---------------------------------------------------------------------------------------------------------------- the texts

def illumina_fastq(rng, n_bytes):
    out, size, i = [], 0, 0
    quals = np.frombuffer(bytes(range(33, 74)), np.uint8)                       # 41 quality letters
    while size < n_bytes:
        rec = (b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n" % (1101 + i // 5000, 1000 + (i * 37) % 30000, 1000 + (i * 101) % 30000) +
               bytes(rng.choice(list(b"ACGT"), size=150).astype(np.uint8)) + b"\n+\n" +
               bytes(rng.choice(quals, size=150, p=np.linspace(1, 8, 41) / np.linspace(1, 8, 41).sum())) + b"\n")
        out.append(rec); size += len(rec); i += 1
    return b"".join(out)[:n_bytes]


# Literal/length symbols (the end-of-block among them, at the longest length) per code length 1, 2, 3, ...: a symbol of length l occurs
# 2^(Lmax - l) times, so the counts are dyadic and every Huffman tree gives exactly these lengths.  The histogram of the 257 lengths and
# the two distance 1s then has a plain tree deeper than the 7 bits a code-length code may take.
CL_LIMIT_TABLES = {
    "cl_limit_14": [1, 1, 1, 1, 1, 1, 0, 0, 2, 1, 11, 13, 1, 34],
    "cl_limit_13": [1, 1, 0, 1, 2, 1, 4, 11, 1, 1, 32, 15, 106],
}


def cl_limit_design(name):
    """-> (Lmax, [length of each of the used literal/length symbols, the end-of-block last])"""
    per_len = CL_LIMIT_TABLES[name]
    lmax = len(per_len)
    lens = [l for l, k in enumerate(per_len, 1) for _ in range(k)]
    assert lens[-1] == lmax and sum(1 << (lmax - l) for l in lens) == 1 << lmax
    return lmax, lens


def cl_limit_texts():
    out = {}
    for seed, name in enumerate(CL_LIMIT_TABLES):
        rng = np.random.default_rng(1400 + seed)
        lmax, lens = cl_limit_design(name)
        values = rng.permutation(256)[:len(lens) - 1].astype(np.uint8)           # (the last symbol of the design is the end-of-block)
        text = np.repeat(values, [1 << (lmax - l) for l in lens[:-1]])
        rng.shuffle(text)
        out[name] = text.tobytes()
    return out


CLUSTER_ROUNDS = {"cluster_first": 0, "cluster_middle": 31, "cluster_last": 62}


def clustered_texts():
    """about 250 values that occur 4 times each (14 bits) all inside ONE aligned 1 KiB round, six heavy values with halving counts
    around them (the rare values' subtree hangs 6 levels down): that round is the most the output ring ever takes.  `cluster_last` is
    62 KiB + 1000 bytes: its cluster is the last, partial round."""
    out = {}
    for seed, (name, rnd) in enumerate(CLUSTER_ROUNDS.items()):
        rng = np.random.default_rng(4800 + seed)
        values = rng.permutation(256).astype(np.uint8)
        heavy = values[:6]
        if name == "cluster_last":
            n = 62 * 1024 + 1000
            cluster = np.repeat(values[6:256], 4)                                # 250 x 4 = the 1000 bytes of the last round
        else:
            n = BLOCK
            cluster = np.concatenate([np.repeat(values[6:250], 4), np.repeat(values[250:256], 8)])   # 244 x 4 + 6 x 8 = a whole round
        n_heavy = n - len(cluster)
        unit = n_heavy // 63
        counts = [unit * (1 << (5 - i)) for i in range(6)]
        counts[0] += n_heavy - sum(counts)
        rest = np.repeat(heavy, counts)
        rng.shuffle(rest)
        rng.shuffle(cluster)
        text = np.concatenate([rest[:rnd * 1024], cluster, rest[rnd * 1024:]])
        assert len(text) == n and (len(cluster) == 1024 or rnd * 1024 + len(cluster) == n)
        out[name] = text.tobytes()
    return out


SHORT_LENGTHS = list(range(1, 71)) + [255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097]


def short_texts():
    rng = np.random.default_rng(70)
    fq = illumina_fastq(rng, 5000)
    out = {}
    for n in SHORT_LENGTHS:
        out[f"two_letter_{n}"] = bytes(rng.choice(list(b"AC"), size=n).astype(np.uint8))
        out[f"fastq_{n}"] = fq[:n]
    out["two_symbols_2"], out["two_symbols_3"], out["two_symbols_5"] = b"GT", b"GTG", b"TGTTG"
    return out


def coded_bytes(piece):
    """the bytes of the piece's member in the coded form under plain Huffman codes (both trees must fit their limits)"""
    hist = piece_histogram(piece)
    cost, depth, lit = plain_huffman(hist)
    cl_cost, cl_depth, cl = plain_huffman(code_length_histogram(lit + [1, 1]))
    assert depth <= 15 and cl_depth <= 7
    ncl = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
    return 18 + (17 + 3 * ncl + cl_cost + cost + 7) // 8 + 8


def break_even_piece():
    """a piece whose coded form takes exactly as many bytes as its stored form, so it must be stored: every byte value twice and one
    value t more times, t searched until the two sizes meet (a step of t moves the difference by fewer than 8 bits)"""
    base = np.repeat(np.arange(256, dtype=np.uint8), 2)
    for t in range(1, 4000):
        piece = np.concatenate([base, np.zeros(t, np.uint8)])
        if coded_bytes(piece.tobytes()) == len(piece) + 31:
            np.random.default_rng(31).shuffle(piece)
            return piece.tobytes()
    raise AssertionError("no break-even piece")


def alignment_texts():
    """5 to 8 members each.  A stored whole piece is 65 311 bytes, 3 modulo 4, so behind the uniform pieces of `random_5` the members
    begin at 3, 2, 1 and 0 modulo 4; the other two texts mix coded members of other lengths in."""
    rng = np.random.default_rng(4004)
    fq = illumina_fastq(rng, 6 * BLOCK)
    rnd = bytes(rng.integers(0, 256, 8 * BLOCK).astype(np.uint8))
    mixed = b"".join((fq if i % 2 else rnd)[i * BLOCK:(i + 1) * BLOCK - (3 if i == 2 else 0)] for i in range(7))
    return {
        "random_5": rnd[:4 * BLOCK + 1001],
        "fastq_6": fq[:5 * BLOCK + 30_003],
        "mixed_8": mixed[:7 * BLOCK] + fq[:4099],
    }


def stride_pieces():
    """the period of stride_text (three whole pieces: FASTQ, uniform bytes, the clustered piece) and its short tail piece"""
    rng = np.random.default_rng(1607)
    return [illumina_fastq(rng, BLOCK), bytes(rng.integers(0, 256, BLOCK).astype(np.uint8)), clustered_texts()["cluster_middle"]], illumina_fastq(rng, 777)


def stride_text(n_members, pad=0):
    """n_members - 1 whole pieces, piece i the (i modulo 3)-th of stride_pieces(), and the tail piece -> uint8 array (+ `pad` zero bytes)"""
    period, tail = stride_pieces()
    assert all(len(p) == BLOCK for p in period)
    reps = (n_members - 1 + 2) // 3
    whole = np.tile(np.frombuffer(b"".join(period), np.uint8), reps)[:(n_members - 1) * BLOCK]
    return np.concatenate([whole, np.frombuffer(tail, np.uint8), np.zeros(pad, np.uint8)])
