// Coverage search for MI355X (gfx950): where on each query an accession hits.  The segmented search (cid_segments.hip) with the windows
// kept in sequence order and the per-window bits kept long enough to become run statistics (include/colorid_hip.h: cid_cover).
//
// A segment is one record: L windows numbered 0 .. L-1, window w covers bases [w, w + k).  Every window has a flag byte: bit 0 VALID (the
// window holds a k-mer; a window with a non-ACGT base stays in place with the bit clear), bit 1 FIRST (the first window of its segment
// with this k-mer).  P[w][c] = window w is VALID and colour c is set in the AND of the n_hash rows of its k-mer; an invalid window is
// absent for every colour and breaks runs.  Per (segment, colour):
//   kmers_hit = windows with P and FIRST       windows_hit = windows with P       n_runs = maximal runs of consecutive windows with P
//   longest_run = windows of the longest run   first_window / last_window = lowest / highest w with P (0xFFFFFFFF: none)
//   bases_covered = |union of [w, w + k) over the windows with P| = windows_hit + sum over interior gaps of min(gap, k - 1)
//                   + (k - 1 if any window hit), a gap being the absent windows between two consecutive runs.
//
// Two launches.  k_cover_rows has the segmented searches' tiles, staging and gather (cid_segwalk.hpp: TileWave; tiles of 64 consecutive
// windows of the whole array) but no segments and so no walk: every lane stores its AND words to rows[window][rs], a window-major matrix
// of u64 — a sub-pass of the wave writes 1 KiB of consecutive bytes.  Invalid windows are not hashed and store zeros.
// k_cover_stats runs one wave per (segment, 64-colour word j).  It walks the segment's tiles in order: lane l loads rows[t*64 + l][j]
// (zero outside the segment, so segments may start and end inside a tile), the wave transposes the 64 x 64 bit block across its lanes, and
// lane c, which then holds the 64 window bits of colour 64j + c, folds them into its statistics with plain bit operations; the state
// (open run, zeros since the last run, counts) is carried in registers from tile to tile.  Lanes hold consecutive colours, so the
// 32-byte cells they write are consecutive.
#include "cid_segwalk.hpp"

namespace cid {

template <int LOG_LPR, bool NARROW>
__global__ __launch_bounds__(kBlock) void k_cover_rows(CoverParams q) {
    extern __shared__ __align__(16) uint8_t smem[];
    const SearchParams &p = q.s;
    const TileWave<LOG_LPR, NARROW> w(p, smem);   // (a lane past the row's real width loads nothing and stores zeros)

    for (uint64_t tile = w.w0; tile < w.w1; ++tile) {
        const uint64_t first = tile * kWave;
        const uint32_t n_live = p.n_kmers - first < (uint64_t)kWave ? (uint32_t)(p.n_kmers - first) : (uint32_t)kWave;
        const bool valid = (uint32_t)w.lane < n_live && (!q.flags || (q.flags[first + w.lane] & 1u));
        const uint64_t vmask = __ballot(valid);   // wave-uniform: bit i = window first + i holds a k-mer
        stage_and_hash(w.img, w.ridx, p.kmers, p.codes, p.n_kmers, first, p.k, p.n_hash, p.mod, w.lane, !valid);
#pragma unroll 1
        for (int sub = 0; sub < w.LPR; ++sub) {
            const int kk = w.kk(sub);
            if ((uint32_t)kk >= n_live) continue;
            V16 a{0, 0};
            uint32_t zm;
            if (((vmask >> kk) & 1ull) && w.col_live) a = gather_and<NARROW, false>(p.mat, p.rs, w.ridx, kk, w.col_word, p.n_hash, zm);
            uint64_t *dst = q.rows + (first + (uint32_t)kk) * p.rs + w.col_word;
            if constexpr (NARROW) *dst = a.x;
            else *reinterpret_cast<ulonglong2 *>(dst) = make_ulonglong2(a.x, a.y);
        }
    }
}

struct CoverState {
    uint32_t kmers = 0, wins = 0, gaps = 0, runs = 0, longest = 0;
    uint32_t first = 0xFFFFFFFFu, last = 0xFFFFFFFFu;
    uint32_t open = 0;    // windows of the run that reaches the end of what has been seen (0: the last window seen was absent)
    uint32_t zeros = 0;   // absent windows since the last run ended (those before the first run are dropped when it starts)
};

// 64 more windows of one colour, bit i = window base + i (base wraps below zero for the bits in front of the segment, which are zero).
// The loop walks the word run by run; its shifts stay below 64 and it never counts the zeros of zero: a word of all zeros or all ones
// is taken whole, and past bit `pos` > 0 the shifted word has zeros on top, so its complement has a set bit.
__device__ __forceinline__ void cover_word(CoverState &st, uint64_t x, uint64_t first_mask, uint32_t base, uint32_t gap_cap) {
    if (x == 0) { st.open = 0; st.zeros += 64u; return; }
    st.kmers += (uint32_t)__popcll(x & first_mask);
    st.wins += (uint32_t)__popcll(x);
    if (st.first == 0xFFFFFFFFu) st.first = base + (uint32_t)__builtin_ctzll(x);
    st.last = base + 63u - (uint32_t)__builtin_clzll(x);
    auto ones = [&](uint32_t n) {
        if (st.open == 0) {   // a run starts: the gap behind it is interior iff a run came before
            if (st.runs) st.gaps += st.zeros < gap_cap ? st.zeros : gap_cap;
            ++st.runs;
            st.zeros = 0;
        }
        st.open += n;
        if (st.open > st.longest) st.longest = st.open;
    };
    if (x == ~0ull) { ones(64u); return; }
    uint32_t pos = 0;
    while (pos < 64u) {
        const uint64_t rem = x >> pos;
        if (rem & 1ull) {
            const uint32_t n = (uint32_t)__builtin_ctzll(~rem);
            ones(n);
            pos += n;
        } else {
            const uint32_t n = rem ? (uint32_t)__builtin_ctzll(rem) : 64u - pos;
            st.open = 0;
            st.zeros += n;
            pos += n;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_cover_stats(CoverParams q) {
    const SearchParams &p = q.s;
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t g = wave_uniform((uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6));   // this wave's (segment, word)
    if (g >= q.n_segs * p.w64) return;
    const uint64_t s = g / p.w64;
    const uint32_t j = (uint32_t)(g % p.w64);
    const uint64_t a = wave_uniform(q.seg_off[s]), b = wave_uniform(q.seg_off[s + 1]);

    CoverState st;
    if (b > a) {
        for (uint64_t t = a / kWave; t * kWave < b; ++t) {
            const uint64_t w = t * kWave + lane;
            const bool in = w >= a && w < b;
            uint64_t x = in ? q.rows[w * p.rs + j] : 0ull;
            const uint32_t fl = (in && q.flags) ? q.flags[w] : 3u;
            const uint64_t first_mask = __ballot((fl & 2u) != 0);   // wave-uniform; outside the segment x is zero whatever it says
            x = transpose_bits64(x, lane);
            cover_word(st, x, first_mask, (uint32_t)(t * kWave - a), p.k - 1u);
        }
    }
    const uint32_t c = j * 64u + lane;
    if (c < p.n_colors) {
        uint4 *o = reinterpret_cast<uint4 *>(q.out + (s * p.n_colors + c) * 8u);
        o[0] = make_uint4(st.kmers, st.wins, st.wins + st.gaps + (st.wins ? p.k - 1u : 0u), st.runs);
        o[1] = make_uint4(st.longest, st.first, st.last, 0u);
    }
}

hipError_t launch_cover_rows(const CoverParams &q, hipStream_t stream) {
    CID_LAUNCH_TILES(k_cover_rows, q.s, false, stream, q);
}

hipError_t launch_cover_stats(const CoverParams &q, hipStream_t stream) {
    const uint64_t waves = q.n_segs * q.s.w64;
    if (waves == 0) return hipSuccess;
    const uint64_t grid = (waves + kBlock / kWave - 1) / (kBlock / kWave);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cover_stats, dim3((uint32_t)grid), dim3(kBlock), 0, stream, q);
    return hipGetLastError();
}

}  // namespace cid
