// Block-gzip (BGZF) members WRITTEN on the device: the mirror image of cid_inflate.hip, for read_id --taxon (the kept reads leave the
// GPU compressed; gzip at the default level on the host's cores would cost several times the classification).
//   text in HBM, cut every 65 280 bytes (htslib's block size: a stored block always fits a 64 KiB member)
//     --k_bgzf_deflate, one wave per piece--> a whole member in a fixed slot: gzip header with the "BC" field | DEFLATE | CRC-32 | ISIZE
//     --one scan over the members' lengths, k_bgzf_gather--> the members back to back.
// The DEFLATE stream is ONE dynamic-Huffman block over literals and end-of-block (no LZ77 matches: DESIGN.md §5 says what that costs
// against zlib), or one stored block when that would not be smaller — so no member is longer than its text + 31 bytes:
//   histogram of the piece's bytes in LDS -> Huffman code lengths (rank sort by all lanes, the two-queue merge by one lane, depths by
//   all lanes), limited to 15 bits by moving leaves down until the Kraft sum is exactly one (zlib refuses an incomplete or
//   over-subscribed literal/length set) -> canonical codes -> the same for the code-length alphabet (7 bits) -> every size is known
//   before a bit is written, BSIZE included -> the literals coded 1 KiB a round: a lane looks up its 16 bytes, a wave prefix sum over
//   the lanes' bit counts gives every lane its bit offset, the lanes OR their bits into a ring of 512 words in LDS, and the words a
//   round completes leave as one coalesced store.
// The output is a function of the text alone: LDS atomics only add counts and OR disjoint bits, no atomic decides a byte's position.
//
// cid_bgzf_deflate_lz (k_bgzf_deflate_lz, opt-in: read_id --taxon --gz-matches) is the same decomposition with an LZ77 match finder per
// wave in front of the coder:
//   the piece in stripes of 64 positions, a lane per position: the lane hashes its next 4 bytes, reads the last earlier position with
//   that hash from a table in LDS (4096 words; positions of EARLIER stripes only, entered by atomicMax — the largest position wins
//   whichever lane arrives first — and cleared between the pieces a wave takes in turn), compares the bytes there with its own (a stale
//   or colliding entry fails this and costs ratio, never correctness) and extends the match 4 bytes a step up to 258 or the piece's end
//   -> a match is kept when this piece's literal code would spend more bits on its bytes (judged by its first four) than two codes
//   and the extra bits of its length and distance cost -> greedy selection left to right over the stripe by ballot: the first lane
//   that holds a match takes it, the lanes it covers drop out, the first one behind it goes on; a stripe that a match covers whole is skipped -> a token per literal / match
//   (4 bytes: literal, or 1 << 23 | length - 3 << 15 | distance - 1) to scratch in HBM, 65 280 tokens x 4 = 261 120 bytes per
//   WORKGROUP IN FLIGHT (6 x CUs of them at most, 383 MiB on 256 CUs; min(members, 6 x CUs) x 261 120 bytes in general), from the
//   ctx's block cache -> two histograms (literal/length 286, distance 30), two codes of <= 15 bits, the code-length code over the
//   HLIT + HDIST lengths (trailing unused symbols trimmed, no run codes) -> the member's size; the size of TODAY's member for the same
//   piece is computed beside it by the same code as k_bgzf_deflate, and the LZ form is written only when it is strictly shorter:
//   otherwise the member is k_bgzf_deflate's, byte for byte -> the tokens coded 256 a round through the same ring.
//
// Both kernels are templates over WHERE the pieces lie: DefContig — piece mi at mi x 65 280 of one text, the form above — or DefTable —
// an (offset, length) per piece, for several texts in one buffer that are each cut from their own start (cid_bgzf_deflate_segments,
// cid_fastq_split: read_id --split; no member spans two texts).  Everything behind the piece's (src, n) is the same code.
#include <cstring>

#include <vector>

#include "cid_api_common.hpp"
#include "cid_scan.hpp"

using cid::fail;

namespace cid {

constexpr uint32_t kDefBlock = 65280;            // text bytes per member
constexpr uint32_t kDefSlot = kDefBlock + 32;    // a member's slot: text + 31 at most, rounded up to whole words
constexpr uint32_t kDefStage = 512;              // ring of output words in LDS: a round adds 64 lanes x 16 bytes x 15 bits = 480 words at most
                                                 // (k_bgzf_deflate_lz: 64 lanes x 4 tokens x (15 + 5 + 15 + 13) bits = 384 words at most)
constexpr uint32_t kDefLit = 257;                // literals + end-of-block
constexpr uint32_t kDefLens = kDefLit + 2;       // + two distance codes of one bit (never used; a complete set, as zlib writes it)

struct CrcShift1K { uint32_t m[32]; };   // column j: the CRC register 1 << j after 1024 zero bytes

struct DefLds {
    uint32_t freq[kDefLit + 3];
    uint32_t tab[kDefLit + 3];     // per literal: its code, bit-reversed (DEFLATE packs Huffman codes from the top bit) | length << 16
    uint8_t len[kDefLens + 5];
    uint32_t clfreq[20], cltab[20];
    uint8_t cllen[20];
    uint32_t blc[17], next[17];
    uint32_t stage[kDefStage];
    union {
        uint32_t crc[1024];                                              // slicing-by-4 tables
        struct { uint32_t w[572]; uint16_t parent[572], order[288]; } b;   // the tree: leaves by ascending weight, then the merged nodes (286 symbols at most)
    } u;
};

__device__ __forceinline__ uint32_t def_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Code lengths (<= maxbits) and canonical codes of the symbols with freq != 0; false when fewer than two symbols are used (no caller
// here can get there: a piece holds a literal and the end-of-block; the lengths hold a zero or two values).  The whole wave calls it.
__device__ bool def_huffman(const uint32_t *freq, uint32_t n, uint32_t maxbits, uint8_t *len, uint32_t *tab, DefLds &S, uint32_t lane) {
    uint32_t cnt = 0;
    for (uint32_t s = lane; s < n; s += 64) cnt += freq[s] != 0;
    cnt = def_wave_sum(cnt);
    if (cnt < 2) return false;
    // rank of every used symbol by (weight, symbol)
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t f = freq[s];
        len[s] = 0;
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            r += (g != 0) && (g < f || (g == f && j < s));
        }
        S.u.b.order[r] = (uint16_t)s;
        S.u.b.w[r] = f;
    }
    if (lane < 17) S.blc[lane] = 0;
    __syncthreads();
    // the two-queue merge: leaves and merged nodes are both in ascending weight, the two lightest heads make the next node
    const uint32_t root = 2 * cnt - 2;
    if (lane == 0) {
        uint32_t i = 0, j = cnt;
        for (uint32_t k = cnt; k <= root; ++k) {
            uint32_t pick[2];
            for (int t = 0; t < 2; ++t) pick[t] = (i < cnt && (j >= k || S.u.b.w[i] <= S.u.b.w[j])) ? i++ : j++;
            S.u.b.w[k] = S.u.b.w[pick[0]] + S.u.b.w[pick[1]];
            S.u.b.parent[pick[0]] = (uint16_t)k;
            S.u.b.parent[pick[1]] = (uint16_t)k;
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < cnt; i += 64) {
        uint32_t d = 0;
        for (uint32_t node = i; node != root; node = S.u.b.parent[node]) ++d;
        atomicAdd(&S.blc[d < maxbits ? d : maxbits], 1u);
    }
    __syncthreads();
    if (lane == 0) {
        // leaves deeper than maxbits were counted AT maxbits: the set is over-subscribed by `total - 2^maxbits` codes of that length.
        // Each turn takes one leaf off the deepest level, moves a leaf of the nearest shallower level one down and hangs the first
        // beside it: the Kraft sum falls by 2^-maxbits, until it is exactly one.
        uint32_t total = 0;
        for (uint32_t l = 1; l <= maxbits; ++l) total += S.blc[l] << (maxbits - l);
        while (total > (1u << maxbits)) {
            S.blc[maxbits] -= 1;
            for (uint32_t l = maxbits - 1; l > 0; --l)
                if (S.blc[l]) { S.blc[l] -= 1; S.blc[l + 1] += 2; break; }
            --total;
        }
        uint32_t code = 0;
        S.blc[0] = 0;
        for (uint32_t l = 1; l <= maxbits; ++l) { code = (code + S.blc[l - 1]) << 1; S.next[l] = code; }
    }
    __syncthreads();
    // the heaviest symbol takes the shortest length
    for (uint32_t i = lane; i < cnt; i += 64) {
        const uint32_t p = cnt - 1 - i;
        uint32_t acc = 0, l = 1;
        for (; l < maxbits; ++l) { acc += S.blc[l]; if (p < acc) break; }
        len[S.u.b.order[i]] = (uint8_t)l;
    }
    __syncthreads();
    // canonical codes: symbols of one length count up in symbol order
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t s = base + lane, L = s < n ? len[s] : 0u;
        uint64_t todo = __ballot(L != 0);
        uint32_t code = 0;
        while (todo) {
            const uint32_t Lf = (uint32_t)__shfl((int)L, __builtin_ctzll(todo), 64);
            const uint64_t m = __ballot(L == Lf);
            const uint32_t nx = S.next[Lf];
            if (L == Lf) code = nx + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) S.next[Lf] = nx + (uint32_t)__builtin_popcountll(m);
            __syncthreads();
            todo &= ~m;
        }
        if (s < n) tab[s] = L ? ((__brev(code) >> (32 - L)) | (L << 16)) : 0u;
    }
    __syncthreads();
    return true;
}

struct DefSink {
    uint32_t *stage, *outw;
    uint32_t bitpos, flushed;   // bits written so far; words already in the slot
};
// `v` (no bit set at or above its length) at bit `pos` of the member
__device__ __forceinline__ void def_deposit(uint32_t *stage, uint64_t v, uint32_t pos) {
    const uint32_t sh = pos & 31u, w = pos >> 5;
    const uint64_t lo = v << sh;
    const uint32_t a = (uint32_t)lo, b = (uint32_t)(lo >> 32), hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
    if (a) atomicOr(&stage[w & (kDefStage - 1)], a);
    if (b) atomicOr(&stage[(w + 1) & (kDefStage - 1)], b);
    if (hi) atomicOr(&stage[(w + 2) & (kDefStage - 1)], hi);
}
// every lane appends up to four pieces of bits, lane 0's first; at most 480 words a call
__device__ __forceinline__ void def_put(DefSink &k, uint32_t lane, const uint64_t v[4], const uint32_t nb[4]) {
    const uint32_t tot = nb[0] + nb[1] + nb[2] + nb[3];
    uint32_t incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    uint32_t pos = k.bitpos + incl - tot;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (nb[q]) def_deposit(k.stage, v[q], pos);
        pos += nb[q];
    }
    k.bitpos += (uint32_t)__shfl((int)incl, 63, 64);
    __syncthreads();
    const uint32_t wend = k.bitpos >> 5;
    for (uint32_t w = k.flushed + lane; w < wend; w += 64) {
        k.outw[w] = k.stage[w & (kDefStage - 1)];
        k.stage[w & (kDefStage - 1)] = 0;
    }
    k.flushed = wend;
    __syncthreads();
}

__device__ __forceinline__ uint32_t def_load4(const uint8_t *p, uint32_t at, uint32_t n) {   // bytes at .. at + 3 of a piece of n bytes, zeros behind it
    if (at + 4 <= n) { uint32_t w; __builtin_memcpy(&w, p + at, 4); return w; }
    uint32_t w = 0;
    for (uint32_t i = 0; i < 4 && at + i < n; ++i) w |= (uint32_t)p[at + i] << (8 * i);
    return w;
}

// ---- CRC-32 (RFC 1952 8): a lane per slice of 1 KiB, the slices aligned to the END of the piece so that every slice but the first is
// whole; slicing by 4; the lanes' registers folded with the "append 1024 zero bytes" operator (as k_bgzf_inflate_wave checks it).  Also
// clears the histograms and the ring for the piece.
__device__ __forceinline__ uint32_t def_crc(DefLds &S, const uint8_t *src, uint32_t n, const CrcShift1K &shift, uint32_t lane) {
    uint32_t *ct = S.u.crc;
    for (uint32_t i = lane; i < 256; i += 64) {
        uint32_t c = i;
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        ct[i] = c;
    }
    __syncthreads();
    for (uint32_t i = lane; i < 256; i += 64) {
        uint32_t c = ct[i];
        for (int t = 1; t < 4; ++t) { c = ct[c & 0xFFu] ^ (c >> 8); ct[256 * t + i] = c; }
    }
    for (uint32_t i = lane; i < kDefLit + 3; i += 64) S.freq[i] = 0;
    for (uint32_t i = lane; i < kDefStage; i += 64) S.stage[i] = 0;
    if (lane < 20) S.clfreq[lane] = 0;
    __syncthreads();
    const uint32_t n_slices = (n + 1023u) / 1024u, first_len = n - (n_slices - 1u) * 1024u;
    uint32_t c = 0;
    if (lane < n_slices) {
        const uint32_t b0 = lane == 0 ? 0u : first_len + (lane - 1u) * 1024u, b1 = lane == 0 ? first_len : b0 + 1024u;
        c = lane == 0 ? 0xFFFFFFFFu : 0u;
        uint32_t i = b0;
        for (; i < b1 && ((b1 - i) & 3u); ++i) c = ct[(c ^ src[i]) & 0xFFu] ^ (c >> 8);
        for (; i < b1; i += 4) {
            uint32_t wd;
            __builtin_memcpy(&wd, src + i, 4);
            c ^= wd;
            c = ct[768 + (c & 0xFFu)] ^ ct[512 + ((c >> 8) & 0xFFu)] ^ ct[256 + ((c >> 16) & 0xFFu)] ^ ct[c >> 24];
        }
    }
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t sl = 0; sl < n_slices; ++sl) {
        const uint32_t cs = (uint32_t)__shfl((int)c, (int)sl, 64);
        if (sl == 0) reg = cs;
        else {
            uint32_t rr = 0;
            for (uint32_t j = 0; j < 32; ++j) rr ^= shift.m[j] & (0u - ((reg >> j) & 1u));
            reg = rr ^ cs;
        }
    }
    return reg ^ 0xFFFFFFFFu;
}

__constant__ const uint8_t kDefClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// HCLEN and the bits of a block header whose lengths were counted into clfreq and coded with cllen
__device__ __forceinline__ uint32_t def_header_bits(const uint32_t *clfreq, const uint8_t *cllen, uint32_t lane, uint32_t &ncl) {
    ncl = 4;
    for (uint32_t i = 4; i < 19; ++i) if (cllen[kDefClOrder[i]]) ncl = i + 1;
    const uint32_t bits = lane < 19 ? clfreq[lane] * cllen[lane] : 0u;
    return def_wave_sum(bits) + 17u + 3u * ncl;
}

struct DefPlan { bool coded; uint32_t ncl, total; };   // the literal-only member of a piece: coded or stored, HCLEN, its bytes

// the piece's literal histogram, its two codes (S.len / S.tab, S.cllen / S.cltab) and the coded-versus-stored decision
__device__ __forceinline__ DefPlan def_plan(DefLds &S, const uint8_t *src, uint32_t n, uint32_t lane) {
    // ---- histogram of the piece (coalesced: a lane takes 4 bytes of every 256)
    for (uint32_t at = lane * 4; at < n; at += 256) {
        const uint32_t w = def_load4(src, at, n), k = n - at < 4 ? n - at : 4;
        for (uint32_t i = 0; i < k; ++i) atomicAdd(&S.freq[(w >> (8 * i)) & 0xFFu], 1u);
    }
    if (lane == 0) S.freq[256] = 1;
    __syncthreads();   // (the CRC tables are done with: the tree takes their place)
    bool coded = def_huffman(S.freq, kDefLit, 15, S.len, S.tab, S, lane);
    uint32_t data_bits = 0, hdr_bits = 0, ncl = 4;
    if (coded) {
        for (uint32_t s = lane; s < kDefLit; s += 64) data_bits += S.freq[s] * S.len[s];
        data_bits = def_wave_sum(data_bits);
        if (lane == 0) { S.len[kDefLit] = 1; S.len[kDefLit + 1] = 1; }
        __syncthreads();
        for (uint32_t s = lane; s < kDefLens; s += 64) atomicAdd(&S.clfreq[S.len[s]], 1u);
        __syncthreads();
        coded = def_huffman(S.clfreq, 19, 7, S.cllen, S.cltab, S, lane);
    }
    if (coded) hdr_bits = def_header_bits(S.clfreq, S.cllen, lane, ncl);
    const uint32_t coded_bytes = 18u + (hdr_bits + data_bits + 7u) / 8u + 8u, stored_bytes = n + 31u;
    const bool use_coded = coded && coded_bytes < stored_bytes;   // not smaller -> stored
    return DefPlan{use_coded, ncl, use_coded ? coded_bytes : stored_bytes};
}

// the gzip header (RFC 1952; the "BC" extra field of the SAM specification 4.1: BSIZE = the member's length - 1), three pieces of 6 bytes
__device__ __forceinline__ void def_gzip_header(uint32_t total, uint64_t h[3]) {
    h[0] = 0x1Full | (0x8Bull << 8) | (8ull << 16) | (4ull << 24);                    // magic, deflate, FEXTRA, mtime 0 (2 of 4 bytes)
    h[1] = (0xFFull << 24) | (6ull << 32);                                            // mtime, xfl 0, os 255, XLEN 6
    h[2] = 0x42ull | (0x43ull << 8) | (2ull << 16) | ((uint64_t)(total - 1u) << 32);  // 'B' 'C' SLEN 2, BSIZE
}

// the gzip header, BFINAL | dynamic | HLIT | HDIST | HCLEN, and the code-length code's lengths
__device__ __forceinline__ void def_put_head(DefSink &sink, uint32_t lane, uint32_t total, uint32_t hlit, uint32_t hdist, uint32_t ncl, const uint8_t *cllen) {
    uint64_t h[3];
    def_gzip_header(total, h);
    uint64_t v[4] = {0, 0, 0, 0};
    uint32_t nb[4] = {0, 0, 0, 0};
    if (lane == 0) {
        v[0] = h[0]; v[1] = h[1]; v[2] = h[2]; nb[0] = nb[1] = nb[2] = 48;
        v[3] = 1ull | (2ull << 1) | ((uint64_t)(hlit - 257u) << 3) | ((uint64_t)(hdist - 1u) << 8) | ((uint64_t)(ncl - 4u) << 13);
        nb[3] = 17;
    }
    def_put(sink, lane, v, nb);
    v[0] = v[1] = v[2] = v[3] = 0; nb[0] = nb[1] = nb[2] = nb[3] = 0;
    if (lane == 0) {
        for (uint32_t i = 0; i < ncl; ++i) v[0] |= (uint64_t)cllen[kDefClOrder[i]] << (3 * i);
        nb[0] = 3 * ncl;
    }
    def_put(sink, lane, v, nb);
}

// the end-of-block (its table entry), zeros up to the byte boundary, CRC-32 and ISIZE; the last, partial word leaves the ring
__device__ __forceinline__ void def_put_tail(DefSink &sink, DefLds &S, uint32_t lane, uint32_t eob, uint32_t crc, uint32_t n) {
    uint64_t v[4] = {0, 0, 0, 0};
    uint32_t nb[4] = {0, 0, 0, 0};
    if (lane == 0) {
        v[0] = eob & 0xFFFFu; nb[0] = eob >> 16;
        nb[1] = (0u - (sink.bitpos + nb[0])) & 7u;             // the stream ends on a byte boundary
        v[2] = (uint64_t)crc | ((uint64_t)n << 32); nb[2] = 64;
    }
    def_put(sink, lane, v, nb);
    if (lane == 0 && (sink.bitpos & 31u)) sink.outw[sink.flushed] = S.stage[sink.flushed & (kDefStage - 1)];
    __syncthreads();
    if (lane == 0) S.stage[sink.flushed & (kDefStage - 1)] = 0;
}

// the literal-only member that def_plan decided on, into its slot
__device__ __forceinline__ void def_write(DefLds &S, uint8_t *slot, const uint8_t *src, uint32_t n, uint32_t crc, const DefPlan &plan, uint32_t lane) {
    if (plan.coded) {
        DefSink sink{S.stage, reinterpret_cast<uint32_t *>(slot), 0u, 0u};
        def_put_head(sink, lane, plan.total, 257u, 2u, plan.ncl, S.cllen);   // HLIT 257, HDIST 2
        uint64_t v[4] = {0, 0, 0, 0};
        uint32_t nb[4] = {0, 0, 0, 0};
        for (uint32_t s = lane * 5; s < lane * 5 + 5 && s < kDefLens; ++s) {
            const uint32_t e = S.cltab[S.len[s]];
            v[0] |= (uint64_t)(e & 0xFFFFu) << nb[0];
            nb[0] += e >> 16;
        }
        def_put(sink, lane, v, nb);
        for (uint32_t base = 0; base < n; base += 1024) {
            const uint32_t at = base + lane * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = 0; nb[q] = 0;
                const uint32_t a = at + 4 * q;
                if (a < n) {
                    const uint32_t w = def_load4(src, a, n), k = n - a < 4 ? n - a : 4;
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint32_t e = S.tab[(w >> (8 * i)) & 0xFFu];
                        v[q] |= (uint64_t)(e & 0xFFFFu) << nb[q];
                        nb[q] += e >> 16;
                    }
                }
            }
            def_put(sink, lane, v, nb);
        }
        def_put_tail(sink, S, lane, S.tab[256], crc, n);
    } else {
        // one stored block: BFINAL | stored, LEN, ~LEN, the bytes
        if (lane == 0) {
            uint64_t h[3];
            def_gzip_header(plan.total, h);
            for (int i = 0; i < 6; ++i) { slot[i] = (uint8_t)(h[0] >> (8 * i)); slot[6 + i] = (uint8_t)(h[1] >> (8 * i)); slot[12 + i] = (uint8_t)(h[2] >> (8 * i)); }
            slot[18] = 1;
            slot[19] = (uint8_t)n; slot[20] = (uint8_t)(n >> 8); slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8);
            uint8_t *t = slot + 23 + n;
            for (int i = 0; i < 4; ++i) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(n >> (8 * i)); }
        }
        for (uint32_t i = lane; i < n; i += 64) slot[23 + i] = src[i];
    }
}

// Where the pieces lie.  DefContig: one text cut every kDefBlock bytes (piece mi at mi * kDefBlock, the last one shorter).  DefTable: a
// table of (offset, length) per piece — several texts in one buffer, each cut from ITS start (cid_bgzf_deflate_segments,
// cid_fastq_split); every offset is a multiple of 16, as every piece of the contiguous form is.
struct DefContig {
    const uint8_t *text;
    uint64_t text_bytes;
    __device__ __forceinline__ const uint8_t *operator()(uint32_t mi, uint32_t &n) const {
        const uint64_t left = text_bytes - (uint64_t)mi * kDefBlock;
        n = left < kDefBlock ? (uint32_t)left : kDefBlock;   // >= 1
        return text + (uint64_t)mi * kDefBlock;
    }
};
struct DefTable {
    const uint8_t *text;
    const uint64_t *piece_off;
    const uint32_t *piece_len;   // 1 .. kDefBlock
    __device__ __forceinline__ const uint8_t *operator()(uint32_t mi, uint32_t &n) const {
        n = piece_len[mi];
        return text + piece_off[mi];
    }
};

template <typename Pieces>
__global__ __launch_bounds__(64) void k_bgzf_deflate(Pieces pieces, uint32_t n_members, uint8_t *slots, uint32_t *member_len, CrcShift1K shift) {
    __shared__ DefLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t mi = blockIdx.x; mi < n_members; mi += gridDim.x) {
        uint32_t n;
        const uint8_t *src = pieces(mi, n);
        uint8_t *slot = slots + (uint64_t)mi * kDefSlot;
        __syncthreads();
        const uint32_t crc = def_crc(S, src, n, shift, lane);
        const DefPlan plan = def_plan(S, src, n, lane);
        def_write(S, slot, src, n, crc, plan, lane);
        if (lane == 0) member_len[mi] = plan.total;
    }
}

// ---- the same with LZ77 matches (RFC 1951 3.2.5) ----
constexpr uint32_t kLzHash = 4096;       // words of the table of last positions
constexpr uint32_t kLzMin = 4;           // the shortest match taken (the hash covers 4 bytes)
constexpr uint32_t kLzMax = 258;
constexpr uint32_t kLzWindow = 32768;
constexpr uint32_t kLzLit = 286;         // literal/length symbols
constexpr uint32_t kLzDist = 30;         // distance symbols
constexpr uint32_t kLzCodeBits = 12;     // what a match's length and distance codes are taken to cost when a candidate is weighed
constexpr uint32_t kLzMatch = 1u << 23;  // a token: a literal, or kLzMatch | (length - 3) << 15 | (distance - 1)
// LDS per workgroup: DefLds 8 804 + histograms 1 280 + table 16 384 = 26 468 bytes -> 6 workgroups (waves) per CU of 160 KiB
constexpr uint32_t kLzWavesPerCu = 6;

struct LzLds {
    DefLds d;
    uint32_t lfreq[288], dfreq[32];
    union {
        uint32_t head[kLzHash];   // per hash: 1 + the last position entered (0: none), of the stripes before the current one
        struct {                  // once the tokens are found: the codes of the LZ form
            uint32_t ltab[288], dtab[32], clfreq[20], cltab[20];
            uint8_t llen[288], dlen[32], cllen[20];
        } c;
    } u;
};
static_assert(sizeof(LzLds) * kLzWavesPerCu <= 160u * 1024u, "k_bgzf_deflate_lz: the grid assumes 6 workgroups per CU");

// length - 3 (0 .. 255) -> its symbol, the number of extra bits and their value (RFC 1951 3.2.5: 258 is symbol 285 without extra bits)
__device__ __forceinline__ uint32_t lz_len_sym(uint32_t m, uint32_t &eb, uint32_t &ex) {
    eb = 0; ex = 0;
    if (m < 8) return 257u + m;
    if (m == 255) return 285u;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(m);   // 3 .. 7
    eb = k - 2u;
    ex = m & ((1u << eb) - 1u);
    return 257u + 4u * eb + 4u + ((m >> eb) & 3u);
}
// distance - 1 (0 .. 32 767) -> the same
__device__ __forceinline__ uint32_t lz_dist_sym(uint32_t m, uint32_t &eb, uint32_t &ex) {
    eb = 0; ex = 0;
    if (m < 4) return m;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(m);   // 2 .. 14
    eb = k - 1u;
    ex = m & ((1u << eb) - 1u);
    return 2u * k + ((m >> eb) & 1u);
}
__device__ __forceinline__ uint32_t lz_len_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
__device__ __forceinline__ uint32_t lz_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }

template <typename Pieces>
__global__ __launch_bounds__(64) void k_bgzf_deflate_lz(Pieces pieces, uint32_t n_members, uint8_t *slots, uint32_t *member_len, uint32_t *tokens,
                                                        CrcShift1K shift) {
    __shared__ LzLds L;
    DefLds &S = L.d;
    const uint32_t lane = threadIdx.x;
    uint32_t *tok = tokens + (uint64_t)blockIdx.x * kDefBlock;   // this workgroup's tokens: one per text byte at most
    for (uint32_t mi = blockIdx.x; mi < n_members; mi += gridDim.x) {
        uint32_t n;
        const uint8_t *src = pieces(mi, n);
        uint8_t *slot = slots + (uint64_t)mi * kDefSlot;
        __syncthreads();
        const uint32_t crc = def_crc(S, src, n, shift, lane);
        const DefPlan plain = def_plan(S, src, n, lane);   // today's member for this piece: the form to beat
        // ---- the tokens
        for (uint32_t i = lane; i < kLzHash; i += 64) L.u.head[i] = 0;
        for (uint32_t i = lane; i < 288; i += 64) L.lfreq[i] = 0;
        if (lane < 32) L.dfreq[lane] = 0;
        __syncthreads();
        uint32_t next_free = 0, ntok = 0, nmatch = 0;   // the first position no token covers yet; tokens and matches so far (the same in every lane)
        for (uint32_t base = 0; base < n; base += 64) {
            if (next_free >= base + 64) continue;   // a match covers the stripe whole
            const uint32_t p = base + lane;
            const bool valid = p < n, can = p + kLzMin <= n;   // (the zeros def_load4 pads with are not text: no match begins in the last 3 bytes)
            const uint32_t w = valid ? def_load4(src, p, n) : 0u;
            const uint32_t h = (w * 0x9E3779B1u) >> 20;
            const uint32_t cand = can ? L.u.head[h] : 0u;
            __syncthreads();   // every lane has read the table before any lane enters this stripe's positions
            if (can) atomicMax(&L.u.head[h], p + 1u);
            uint32_t len = 0, dist = 0;
            if (cand && p >= next_free) {
                const uint32_t c = cand - 1u;   // < base
                dist = p - c;
                if (dist <= kLzWindow && def_load4(src, c, n) == w) {
                    const uint32_t maxl = n - p < kLzMax ? n - p : kLzMax;
                    len = 4;
                    while (len < maxl) {
                        const uint32_t x = def_load4(src, p + len, n) ^ def_load4(src, c + len, n);
                        if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
                        len += 4;
                    }
                    if (len > maxl) len = maxl;
                    // worth a token?  What the literal code of this piece (S.len, def_plan's) would spend on the match's bytes, judged by
                    // its first four, against a match's two codes (about kLzCodeBits) and its extra bits: the 4-mers of a read's bases
                    // repeat everywhere and cost 2 bits a base as literals — as matches they would make the member longer
                    uint32_t leb, deb, ex;
                    (void)lz_len_sym(len - 3u, leb, ex);
                    (void)lz_dist_sym(dist - 1u, deb, ex);
                    const uint32_t lit4 = S.len[w & 0xFFu] + S.len[(w >> 8) & 0xFFu] + S.len[(w >> 16) & 0xFFu] + S.len[w >> 24];
                    if (lit4 * len <= 4u * (kLzCodeBits + leb + deb)) len = 0;
                }
            }
            // greedy, left to right: the first lane with a match takes it, the lanes it covers drop out
            bool is_tok = valid && p >= next_free, is_match = false;
            uint64_t m = __ballot(len >= kLzMin && p >= next_free);
            while (m) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m), pl = base + l;
                next_free = pl + (uint32_t)__shfl((int)len, (int)l, 64);
                if (lane == l) is_match = true;
                if (p > pl && p < next_free) is_tok = false;
                const uint32_t k = next_free - base;
                m = k >= 64 ? 0ull : m & ~((1ull << k) - 1ull);
            }
            const uint64_t tb = __ballot(is_tok);
            if (is_tok) {
                const uint32_t at = ntok + (uint32_t)__builtin_popcountll(tb & ((1ull << lane) - 1ull));   // < n: a token covers a byte or more
                if (is_match) {
                    uint32_t eb, ex;
                    tok[at] = kLzMatch | ((len - 3u) << 15) | (dist - 1u);
                    atomicAdd(&L.lfreq[lz_len_sym(len - 3u, eb, ex)], 1u);
                    atomicAdd(&L.dfreq[lz_dist_sym(dist - 1u, eb, ex)], 1u);
                } else {
                    tok[at] = w & 0xFFu;
                    atomicAdd(&L.lfreq[w & 0xFFu], 1u);
                }
            }
            ntok += (uint32_t)__builtin_popcountll(tb);
            nmatch += (uint32_t)__builtin_popcountll(__ballot(is_match));
            __syncthreads();   // this stripe's positions are in the table before the next stripe reads it
        }
        if (lane == 0) L.lfreq[256] = 1;
        __syncthreads();   // (the table is done with: the codes take its place; the tokens are in memory)
        // ---- the LZ form's codes and size
        bool lz = nmatch != 0;
        uint32_t hlit = 257, hdist = 1, ncl = 4, lz_bytes = 0;
        if (lz) {
            if (lane < 32) { L.u.c.dlen[lane] = 0; L.u.c.dtab[lane] = 0; }
            if (lane < 20) L.u.c.clfreq[lane] = 0;
            __syncthreads();
            lz = def_huffman(L.lfreq, kLzLit, 15, L.u.c.llen, L.u.c.ltab, S, lane);
        }
        if (lz && !def_huffman(L.dfreq, kLzDist, 15, L.u.c.dlen, L.u.c.dtab, S, lane)) {
            // every match in one distance symbol: that symbol and a second, unused one take the two codes of one bit (a complete set)
            const uint32_t d0 = (uint32_t)__builtin_ctzll(__ballot(lane < kLzDist && L.dfreq[lane < kLzDist ? lane : 0] != 0)), d1 = d0 ? 0u : 1u;
            if (lane == 0) {
                L.u.c.dlen[d0] = 1; L.u.c.dlen[d1] = 1;
                L.u.c.dtab[d0 < d1 ? d0 : d1] = 0u | (1u << 16);
                L.u.c.dtab[d0 < d1 ? d1 : d0] = 1u | (1u << 16);
            }
            __syncthreads();
        }
        if (lz) {
            for (uint32_t s = lane; s < kLzLit; s += 64) if (L.lfreq[s] && s >= hlit) hlit = s + 1;
            if (lane < kLzDist && L.u.c.dlen[lane]) hdist = lane + 1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t a = __shfl_xor(hlit, o, 64), b = __shfl_xor(hdist, o, 64);
                hlit = a > hlit ? a : hlit; hdist = b > hdist ? b : hdist;
            }
            for (uint32_t i = lane; i < hlit + hdist; i += 64) atomicAdd(&L.u.c.clfreq[i < hlit ? L.u.c.llen[i] : L.u.c.dlen[i - hlit]], 1u);
            __syncthreads();
            lz = def_huffman(L.u.c.clfreq, 19, 7, L.u.c.cllen, L.u.c.cltab, S, lane);
        }
        if (lz) {
            uint32_t data_bits = 0;
            for (uint32_t s = lane; s < kLzLit; s += 64) data_bits += L.lfreq[s] * (L.u.c.llen[s] + lz_len_extra(s));
            if (lane < kLzDist) data_bits += L.dfreq[lane] * (L.u.c.dlen[lane] + lz_dist_extra(lane));
            data_bits = def_wave_sum(data_bits);
            const uint32_t hdr_bits = def_header_bits(L.u.c.clfreq, L.u.c.cllen, lane, ncl);
            lz_bytes = 18u + (hdr_bits + data_bits + 7u) / 8u + 8u;
            lz = lz_bytes < plain.total;   // only when strictly shorter than today's member
        }
        if (lz) {
            DefSink sink{S.stage, reinterpret_cast<uint32_t *>(slot), 0u, 0u};
            def_put_head(sink, lane, lz_bytes, hlit, hdist, ncl, L.u.c.cllen);
            uint64_t v[4] = {0, 0, 0, 0};
            uint32_t nb[4] = {0, 0, 0, 0};
            for (uint32_t i = lane * 5; i < lane * 5 + 5 && i < hlit + hdist; ++i) {   // 316 lengths at most: 5 a lane
                const uint32_t e = L.u.c.cltab[i < hlit ? L.u.c.llen[i] : L.u.c.dlen[i - hlit]];
                v[0] |= (uint64_t)(e & 0xFFFFu) << nb[0];
                nb[0] += e >> 16;
            }
            def_put(sink, lane, v, nb);
            for (uint32_t base = 0; base < ntok; base += 256) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = 0; nb[q] = 0;
                    const uint32_t i = base + lane * 4 + q;
                    if (i < ntok) {
                        const uint32_t t = tok[i];
                        if (t & kLzMatch) {
                            uint32_t eb, ex;
                            uint32_t e = L.u.c.ltab[lz_len_sym((t >> 15) & 0xFFu, eb, ex)];
                            v[q] = e & 0xFFFFu; nb[q] = e >> 16;
                            v[q] |= (uint64_t)ex << nb[q]; nb[q] += eb;
                            e = L.u.c.dtab[lz_dist_sym(t & 0x7FFFu, eb, ex)];
                            v[q] |= (uint64_t)(e & 0xFFFFu) << nb[q]; nb[q] += e >> 16;
                            v[q] |= (uint64_t)ex << nb[q]; nb[q] += eb;
                        } else {
                            const uint32_t e = L.u.c.ltab[t];
                            v[q] = e & 0xFFFFu; nb[q] = e >> 16;
                        }
                    }
                }
                def_put(sink, lane, v, nb);
            }
            def_put_tail(sink, S, lane, L.u.c.ltab[256], crc, n);
        } else {
            def_write(S, slot, src, n, crc, plain, lane);
        }
        if (lane == 0) member_len[mi] = lz ? lz_bytes : plain.total;
    }
}

// member i's bytes from its slot to members + off[i]; whole words of the destination, the source read through two aligned words
__global__ __launch_bounds__(256) void k_bgzf_gather(const uint8_t *slots, const uint32_t *member_len, const uint64_t *off, uint32_t n_members, uint8_t *members,
                                                     uint64_t *total) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && total) *total = off[n_members];
    for (uint32_t mi = blockIdx.x; mi < n_members; mi += gridDim.x) {
        const uint8_t *src = slots + (uint64_t)mi * kDefSlot;
        uint8_t *dst = members + off[mi];
        const uint32_t len = member_len[mi];
        const uint32_t head = (uint32_t)((0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u) < len ? (uint32_t)((0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u) : len;
        const uint32_t words = (len - head) / 4, tail = head + words * 4;
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        if (threadIdx.x < len - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(src);   // (slots are whole words; `head` is the source's misalignment)
        uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
        for (uint32_t k = threadIdx.x; k < words; k += 256) {
            const uint32_t a = sw[k], b = head ? sw[k + 1] : 0u;   // (k + 1 stays inside the slot: head > 0 leaves bytes behind word k)
            dw[k] = head ? (a >> (8 * head)) | (b << (32 - 8 * head)) : a;
        }
    }
}

struct DefLenIn {   // the members' lengths and a zero behind them
    const uint32_t *p;
    uint64_t n;
    __device__ uint64_t operator()(uint64_t i) const { return i < n ? p[i] : 0ull; }
};

// ---- several texts in one call (cid_bgzf_deflate_segments, cid_fastq_split): segment s holds seg_len[s] bytes at base[s] of one buffer and
// is cut every kDefBlock bytes from ITS start, so no member spans two segments.  Two scans over the segments give every segment its base
// (the lengths rounded up to 16: every piece then starts on a multiple of 16, as every piece of the contiguous form does — kDefBlock is
// 16 x 4 080) and the index of its first piece; a zero behind the last segment leaves the two totals in element n.
struct DefSegRoomIn {
    const uint64_t *len;
    uint64_t n;
    __device__ uint64_t operator()(uint64_t i) const { return i < n ? (len[i] + 15ull) & ~15ull : 0ull; }
};
struct DefSegPiecesIn {
    const uint64_t *len;
    uint64_t n;
    __device__ uint64_t operator()(uint64_t i) const { return i < n ? (len[i] + kDefBlock - 1) / kDefBlock : 0ull; }
};
// piece p: the segment it belongs to is the last one whose first piece is not behind p (empty segments repeat their successor's index
// and are passed over); its text begins (p - first) x kDefBlock into the segment
__global__ __launch_bounds__(256) void k_bgzf_piece_table(const uint64_t *seg_len, const uint64_t *base, const uint64_t *piece_first, uint32_t n_segs,
                                                          uint32_t n_pieces, uint64_t *piece_off, uint32_t *piece_len) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pieces) return;
    uint32_t lo = 0, hi = n_segs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (piece_first[mid] <= p) lo = mid; else hi = mid;
    }
    const uint64_t at = (uint64_t)(p - (uint32_t)piece_first[lo]) * kDefBlock, left = seg_len[lo] - at;
    piece_off[p] = base[lo] + at;
    piece_len[p] = left < kDefBlock ? (uint32_t)left : kDefBlock;
}
// seg_off[s] = where segment s's members begin in the gathered output (element n_segs: the total)
__global__ __launch_bounds__(256) void k_bgzf_seg_off(const uint64_t *member_off, const uint64_t *piece_first, uint32_t n_segs, uint64_t *seg_off) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= n_segs) seg_off[s] = member_off[piece_first[s]];
}

static CrcShift1K make_crc_shift_1k() {
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        tab[i] = c;
    }
    CrcShift1K s;
    for (uint32_t j = 0; j < 32; ++j) {
        uint32_t c = 1u << j;
        for (int i = 0; i < 1024; ++i) c = tab[c & 0xFFu] ^ (c >> 8);
        s.m[j] = c;
    }
    return s;
}

hipError_t warm_deflate() {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_bgzf_deflate<DefContig>));
    return e != hipSuccess ? e : hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_bgzf_deflate_lz<DefContig>));
}

size_t bgzf_deflate_members(size_t text_bytes) { return (text_bytes + kDefBlock - 1) / kDefBlock; }

// the n pieces `pieces` names -> d_members, d_member_len [n], *d_total; with d_seg_off, also where the members of each of n_segs segments
// begin (d_piece_first [n_segs + 1]: a segment's first piece).  Scratch from the ctx's block cache, returned behind the kernels on the same stream
template <typename Pieces>
static int deflate_run(cid_ctx *c, hipStream_t st, Pieces pieces, size_t n, uint8_t *d_members, uint32_t *d_member_len, uint64_t *d_total, bool matches,
                       const uint64_t *d_piece_first, size_t n_segs, uint64_t *d_seg_off) {
    if (n >= (1ull << 31)) return fail(CID_ERR_UNSUPPORTED, "cid_bgzf_deflate: more than 2^31 members in one call");
    static const CrcShift1K shift = make_crc_shift_1k();
    void *slots = nullptr, *off = nullptr, *state = nullptr, *tokens = nullptr;
    int rc;
    // (the LZ kernel's LDS lets kLzWavesPerCu workgroups share a CU, k_bgzf_deflate's 9 KiB sixteen)
    const unsigned grid = (unsigned)std::min<size_t>(n, (size_t)c->n_cu * (matches ? kLzWavesPerCu : 16u));
    if ((rc = ctx_alloc(c, n * kDefSlot + 16, &slots))) return rc;
    if ((rc = ctx_alloc(c, (n + 1) * 8, &off))) { ctx_free(c, slots); return rc; }
    if ((rc = ctx_alloc(c, scan_state_words(n + 1) * 8, &state))) { ctx_free(c, slots); ctx_free(c, off); return rc; }
    if (matches && (rc = ctx_alloc(c, (size_t)grid * kDefBlock * 4, &tokens))) { ctx_free(c, slots); ctx_free(c, off); ctx_free(c, state); return rc; }
    auto done = [&](int code) { ctx_free(c, slots); ctx_free(c, off); ctx_free(c, state); if (tokens) ctx_free(c, tokens); return code; };
    if (matches)
        hipLaunchKernelGGL(k_bgzf_deflate_lz<Pieces>, dim3(grid), dim3(64), 0, st, pieces, (uint32_t)n, (uint8_t *)slots, d_member_len, (uint32_t *)tokens, shift);
    else
        hipLaunchKernelGGL(k_bgzf_deflate<Pieces>, dim3(grid), dim3(64), 0, st, pieces, (uint32_t)n, (uint8_t *)slots, d_member_len, shift);
    hipError_t e = hipGetLastError();
    // off[i] = the bytes of the members before i (the element behind the last one is zero: its prefix is the total)
    if (e == hipSuccess) e = scan_launch(DefLenIn{d_member_len, n}, ScanOutU64{(uint64_t *)off, 0ull}, n + 1, (uint64_t *)state, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_bgzf_gather, dim3((unsigned)std::min<size_t>(n, 65535)), dim3(256), 0, st, (const uint8_t *)slots, (const uint32_t *)d_member_len,
                           (const uint64_t *)off, (uint32_t)n, d_members, d_total);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d_seg_off) {
        hipLaunchKernelGGL(k_bgzf_seg_off, dim3((unsigned)((n_segs + 256) / 256)), dim3(256), 0, st, (const uint64_t *)off, d_piece_first, (uint32_t)n_segs, d_seg_off);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate: %s", hipGetErrorString(e)));
    return done(CID_OK);
}

// d_text (16-byte aligned) -> d_members (>= cid_bgzf_deflate_bound bytes), d_member_len [n], *d_total = the members' bytes; scratch from
// the ctx's block cache, returned behind the kernels on the same stream.  matches: k_bgzf_deflate_lz (its tokens: 261 120 bytes per
// workgroup launched, more scratch of the same kind)
int bgzf_deflate_launch(cid_ctx *c, hipStream_t st, const uint8_t *d_text, size_t text_bytes, uint8_t *d_members, uint32_t *d_member_len, uint64_t *d_total,
                        bool matches) {
    const size_t n = bgzf_deflate_members(text_bytes);
    if (n == 0) {
        if (d_total) HIP_TRY(hipMemsetAsync(d_total, 0, 8, st));
        return CID_OK;
    }
    return deflate_run(c, st, DefContig{d_text, (uint64_t)text_bytes}, n, d_members, d_member_len, d_total, matches, nullptr, 0, nullptr);
}

int bgzf_segments_layout(cid_ctx *c, hipStream_t st, const uint64_t *d_seg_len, size_t n_segs, uint64_t *d_base, uint64_t *d_piece_first) {
    if (n_segs >= (1ull << 31)) return fail(CID_ERR_UNSUPPORTED, "cid_bgzf_deflate_segments: more than 2^31 segments in one call");
    void *state = nullptr;
    int rc;
    if ((rc = ctx_alloc(c, scan_state_words(n_segs + 1) * 8, &state))) return rc;
    hipError_t e = scan_launch(DefSegRoomIn{d_seg_len, n_segs}, ScanOutU64{d_base, 0ull}, n_segs + 1, (uint64_t *)state, st);
    if (e == hipSuccess) e = scan_launch(DefSegPiecesIn{d_seg_len, n_segs}, ScanOutU64{d_piece_first, 0ull}, n_segs + 1, (uint64_t *)state, st);
    ctx_free(c, state);
    return e == hipSuccess ? CID_OK : fail(CID_ERR_HIP, "cid_bgzf_deflate_segments: %s", hipGetErrorString(e));
}

int bgzf_deflate_segments_launch(cid_ctx *c, hipStream_t st, const uint8_t *d_text, const uint64_t *d_seg_len, const uint64_t *d_base,
                                 const uint64_t *d_piece_first, size_t n_segs, size_t n_pieces, uint8_t *d_members, uint32_t *d_member_len, uint64_t *d_total,
                                 uint64_t *d_seg_off, bool matches) {
    if (n_pieces == 0) {
        if (d_total) HIP_TRY(hipMemsetAsync(d_total, 0, 8, st));
        if (d_seg_off) HIP_TRY(hipMemsetAsync(d_seg_off, 0, (n_segs + 1) * 8, st));
        return CID_OK;
    }
    if (n_pieces >= (1ull << 31)) return fail(CID_ERR_UNSUPPORTED, "cid_bgzf_deflate: more than 2^31 members in one call");
    void *piece_off = nullptr, *piece_len = nullptr;
    int rc;
    if ((rc = ctx_alloc(c, n_pieces * 8, &piece_off))) return rc;
    if ((rc = ctx_alloc(c, n_pieces * 4, &piece_len))) { ctx_free(c, piece_off); return rc; }
    hipLaunchKernelGGL(k_bgzf_piece_table, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, st, d_seg_len, d_base, d_piece_first, (uint32_t)n_segs,
                       (uint32_t)n_pieces, (uint64_t *)piece_off, (uint32_t *)piece_len);
    const hipError_t e = hipGetLastError();
    rc = e != hipSuccess ? fail(CID_ERR_HIP, "cid_bgzf_deflate_segments: %s", hipGetErrorString(e))
                         : deflate_run(c, st, DefTable{d_text, (const uint64_t *)piece_off, (const uint32_t *)piece_len}, n_pieces, d_members, d_member_len, d_total,
                                       matches, d_piece_first, n_segs, d_seg_off);
    ctx_free(c, piece_off); ctx_free(c, piece_len);
    return rc;
}

}  // namespace cid

extern "C" {

size_t cid_bgzf_deflate_bound(size_t text_bytes) { return text_bytes + 31 * cid::bgzf_deflate_members(text_bytes); }

static int deflate_dev(cid_ctx *c, const uint8_t *d_text, size_t text_bytes, uint8_t *d_members, size_t members_cap, uint64_t *d_members_bytes,
                       uint32_t *d_member_len, size_t *n_members, bool matches) {
    if (!c || !n_members) return fail(CID_ERR_INVALID, "null argument");
    *n_members = cid::bgzf_deflate_members(text_bytes);
    if (text_bytes && (!d_text || !d_members || !d_member_len)) return fail(CID_ERR_INVALID, "null argument");
    if (!cid::aligned16(d_text)) return fail(CID_ERR_INVALID, "cid_bgzf_deflate_dev: the text must be 16-byte aligned");
    if (members_cap < cid_bgzf_deflate_bound(text_bytes))
        return fail(CID_ERR_INVALID, "cid_bgzf_deflate_dev: %zu bytes of room for the members, cid_bgzf_deflate_bound asks for %zu", members_cap,
                    cid_bgzf_deflate_bound(text_bytes));
    HIP_TRY(hipSetDevice(c->device));
    return cid::bgzf_deflate_launch(c, c->stream, d_text, text_bytes, d_members, d_member_len, d_members_bytes, matches);
}

static int deflate_host(cid_ctx *c, const uint8_t *text, size_t text_bytes, uint8_t *members, size_t members_cap, size_t *members_bytes,
                        uint32_t *member_len, size_t *n_members, bool matches) {
    if (!c || !members_bytes || !n_members) return fail(CID_ERR_INVALID, "null argument");
    *members_bytes = 0;
    const size_t n = *n_members = cid::bgzf_deflate_members(text_bytes);
    if (n == 0) return CID_OK;
    if (!text || !members || !member_len) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bound = cid_bgzf_deflate_bound(text_bytes);
    void *d_text = nullptr, *d_out = nullptr, *d_len = nullptr;
    int rc;
    if ((rc = cid::ctx_alloc(c, text_bytes + 16, &d_text))) return rc;
    if ((rc = cid::ctx_alloc(c, bound + 16, &d_out))) { cid::ctx_free(c, d_text); return rc; }
    if ((rc = cid::ctx_alloc(c, n * 4 + 16, &d_len))) { cid::ctx_free(c, d_text); cid::ctx_free(c, d_out); return rc; }
    uint64_t *d_total = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(d_len) + ((n * 4 + 7) & ~(size_t)7));
    auto done = [&](int code) {
        (void)hipStreamSynchronize(c->stream);
        cid::ctx_free(c, d_text); cid::ctx_free(c, d_out); cid::ctx_free(c, d_len);
        return code;
    };
    hipError_t e = hipMemcpyAsync(d_text, text, text_bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate: %s", hipGetErrorString(e)));
    if ((rc = cid::bgzf_deflate_launch(c, c->stream, (const uint8_t *)d_text, text_bytes, (uint8_t *)d_out, (uint32_t *)d_len, d_total, matches))) return done(rc);
    uint64_t total = 0;
    e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(member_len, d_len, n * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate: %s", hipGetErrorString(e)));
    *members_bytes = (size_t)total;
    if (total > members_cap)
        return done(fail(CID_ERR_INVALID, "cid_bgzf_deflate: the members take %llu bytes, the buffer holds %zu (cid_bgzf_deflate_bound: %zu)",
                         (unsigned long long)total, members_cap, bound));
    e = hipMemcpy(members, d_out, (size_t)total, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate: %s", hipGetErrorString(e)));
    return done(CID_OK);
}

int cid_bgzf_deflate_dev(cid_ctx *c, const uint8_t *d_text, size_t text_bytes, uint8_t *d_members, size_t members_cap, uint64_t *d_members_bytes,
                         uint32_t *d_member_len, size_t *n_members) {
    return deflate_dev(c, d_text, text_bytes, d_members, members_cap, d_members_bytes, d_member_len, n_members, false);
}
int cid_bgzf_deflate(cid_ctx *c, const uint8_t *text, size_t text_bytes, uint8_t *members, size_t members_cap, size_t *members_bytes,
                     uint32_t *member_len, size_t *n_members) {
    return deflate_host(c, text, text_bytes, members, members_cap, members_bytes, member_len, n_members, false);
}
int cid_bgzf_deflate_lz_dev(cid_ctx *c, const uint8_t *d_text, size_t text_bytes, uint8_t *d_members, size_t members_cap, uint64_t *d_members_bytes,
                            uint32_t *d_member_len, size_t *n_members) {
    return deflate_dev(c, d_text, text_bytes, d_members, members_cap, d_members_bytes, d_member_len, n_members, true);
}
int cid_bgzf_deflate_lz(cid_ctx *c, const uint8_t *text, size_t text_bytes, uint8_t *members, size_t members_cap, size_t *members_bytes,
                        uint32_t *member_len, size_t *n_members) {
    return deflate_host(c, text, text_bytes, members, members_cap, members_bytes, member_len, n_members, true);
}

size_t cid_bgzf_deflate_segments_bound(size_t text_bytes, size_t n_segs) { return text_bytes + 31 * (text_bytes / cid::kDefBlock + n_segs); }

int cid_bgzf_deflate_segments(cid_ctx *c, const uint8_t *text, const uint64_t *seg_off, size_t n_segs, int matches, uint8_t *members, size_t members_cap,
                              size_t *members_bytes, uint32_t *member_len, uint64_t *seg_member_first, size_t *n_members) {
    if (!c || !members_bytes || !n_members || (n_segs && (!seg_off || !seg_member_first))) return fail(CID_ERR_INVALID, "null argument");
    *members_bytes = 0; *n_members = 0;
    if (n_segs == 0) return CID_OK;
    // every segment's base in the staged text and its first piece: what the two scans give on the device (from there come the tables
    // the kernels read; from here the staging and the sizes, without a readback)
    std::vector<uint64_t> len(n_segs), base(n_segs + 1, 0);
    size_t np = 0;
    for (size_t s = 0; s < n_segs; ++s) {
        if (seg_off[s + 1] < seg_off[s]) return fail(CID_ERR_INVALID, "cid_bgzf_deflate_segments: segment %zu ends before it begins", s);
        len[s] = seg_off[s + 1] - seg_off[s];
        base[s + 1] = base[s] + ((len[s] + 15) & ~(uint64_t)15);
        np += cid::bgzf_deflate_members((size_t)len[s]);
    }
    for (size_t s = 0; s <= n_segs; ++s) seg_member_first[s] = 0;
    const size_t text_bytes = (size_t)(seg_off[n_segs] - seg_off[0]), room = (size_t)base[n_segs];
    if (np == 0) return CID_OK;
    *n_members = np;
    if (!text || !members || !member_len) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint8_t> staged(room);
    for (size_t s = 0; s < n_segs; ++s) if (len[s]) memcpy(staged.data() + base[s], text + seg_off[s], (size_t)len[s]);
    const size_t bound = cid_bgzf_deflate_segments_bound(text_bytes, n_segs);
    std::vector<void *> held;
    auto take = [&](size_t bytes, void **p) { const int rc = cid::ctx_alloc(c, bytes, p); if (!rc) held.push_back(*p); return rc; };
    auto done = [&](int code) {
        (void)hipStreamSynchronize(c->stream);
        for (void *p : held) cid::ctx_free(c, p);
        return code;
    };
    void *d_text = nullptr, *d_seg_len = nullptr, *d_base = nullptr, *d_first = nullptr, *d_out = nullptr, *d_len = nullptr, *d_total = nullptr;
    int rc;
    if ((rc = take(room + 16, &d_text)) || (rc = take(n_segs * 8, &d_seg_len)) || (rc = take((n_segs + 1) * 8, &d_base)) || (rc = take((n_segs + 1) * 8, &d_first)) ||
        (rc = take(bound + 16, &d_out)) || (rc = take(np * 4, &d_len)) || (rc = take(16, &d_total)))
        return done(rc);
    hipStream_t st = c->stream;
    hipError_t e = hipMemcpyAsync(d_text, staged.data(), room, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_seg_len, len.data(), n_segs * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate_segments: %s", hipGetErrorString(e)));
    if ((rc = cid::bgzf_segments_layout(c, st, (const uint64_t *)d_seg_len, n_segs, (uint64_t *)d_base, (uint64_t *)d_first))) return done(rc);
    if ((rc = cid::bgzf_deflate_segments_launch(c, st, (const uint8_t *)d_text, (const uint64_t *)d_seg_len, (const uint64_t *)d_base, (const uint64_t *)d_first, n_segs,
                                                np, (uint8_t *)d_out, (uint32_t *)d_len, (uint64_t *)d_total, nullptr, matches != 0)))
        return done(rc);
    uint64_t total = 0;
    e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(member_len, d_len, np * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(seg_member_first, d_first, (n_segs + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate_segments: %s", hipGetErrorString(e)));
    *members_bytes = (size_t)total;
    if (total > members_cap)
        return done(fail(CID_ERR_INVALID, "cid_bgzf_deflate_segments: the members take %llu bytes, the buffer holds %zu (cid_bgzf_deflate_segments_bound: %zu)",
                         (unsigned long long)total, members_cap, bound));
    e = hipMemcpy(members, d_out, (size_t)total, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(CID_ERR_HIP, "cid_bgzf_deflate_segments: %s", hipGetErrorString(e)));
    return done(CID_OK);
}

}  // extern "C"
