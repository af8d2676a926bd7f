// Segmented perfect search for MI355X (gfx950): many queries' k-mers laid end to end, per query the AND of all its k-mers' rows
// (src/perfect_search.rs:83-110 per segment) and cid_search_perfect's "some row is absent" flag — `search -s -m`, where every record of a
// scheme's multi-FASTA is an allele and the answer per record is C bits, not C counters.
//
// Decomposition, staging and gather are k_search_segments' (cid_segments.hip): tiles of 64 consecutive k-mers of the whole array,
// stage_and_hash, the per-lane binary search of seg_off (ties resolve to the last equal offset), gather_and with the zero mask.  Only where
// the result goes differs.  A wave keeps ONE segment's running AND in registers: every lane its own column words, preset to all ones; a
// dead lane contributes all ones.  When the wave's next tile belongs to another segment, and at the wave's end, the 64 / LPR k-mer groups
// are reduced with __shfl_xor and the lanes of group 0 atomicAnd their one or two u64 words into and_words[cur][.]: no LDS histogram,
// no counters.  A tile that holds a segment boundary ANDs each live lane's words straight into the row of that lane's own segment: at
// most two atomics per lane and sub-pass (64 * LPR lane visits per tile), however many colours hit.  AND is associative and idempotent,
// so segments that span waves, workgroups or launches need nothing but the atomics, and the result is bit-exact in any order.
//
// The caller presets and_words to all ones and the flags to 0; k_perfect_segments_finish then applies the contract: zero words for an
// empty segment, for a flagged one (as cid_search_perfect zeroes them), and for the bits at and above n_colors.
#include "cid_gather.hpp"

namespace cid {

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, kWave), hi = __shfl_xor((uint32_t)(v >> 32), o, kWave);
    return ((uint64_t)hi << 32) | lo;
}

template <int LOG_LPR, bool NARROW>
__global__ __launch_bounds__(kBlock) void k_perfect_segments(PerfectSegmentParams q) {
    extern __shared__ __align__(16) uint8_t smem[];
    const SearchParams &p = q.s;
    constexpr int LPR = 1 << LOG_LPR;
    constexpr int KPW = kWave / LPR;  // k-mers per sub-pass
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;

    uint8_t *wbase = smem + (size_t)wave * p.wave_bytes;
    uint32_t *img = reinterpret_cast<uint32_t *>(wbase);
    uint32_t *ridx = reinterpret_cast<uint32_t *>(wbase + kmer_img_bytes(p.k));
    uint32_t *s_seg = ridx + kWave * p.n_hash;   // [64] the segment of every k-mer of the tile

    const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
    const uint64_t tile0 = (uint64_t)blockIdx.x * p.tiles_per_block;
    const uint64_t tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
    const uint64_t per_wave = (p.tiles_per_block + kBlock / kWave - 1) / (kBlock / kWave);
    const uint64_t w0 = tile0 + (uint64_t)wave * per_wave;
    const uint64_t w1 = w0 + per_wave < tile1 ? w0 + per_wave : tile1;
    const uint32_t col = lane & (LPR - 1);
    const uint32_t col_word = NARROW ? 0u : 2u * col;
    const bool col_live = col_word < p.w64;  // lanes past the row's real width neither load nor store
    const uint32_t seeds = p.n_hash >= 32 ? ~0u : ((1u << p.n_hash) - 1u);

    auto and_into = [&](uint64_t *row, V16 a) {   // all ones change nothing: no atomic
        if (a.x != ~0ull) atomicAnd(reinterpret_cast<unsigned long long *>(&row[col_word]), (unsigned long long)a.x);
        if constexpr (!NARROW)
            if (a.y != ~0ull) atomicAnd(reinterpret_cast<unsigned long long *>(&row[col_word + 1]), (unsigned long long)a.y);
    };

    V16 acc{~0ull, ~0ull};  // this lane's column words of segment `cur`, ANDed over the k-mers this lane has seen
    uint32_t cur = 0;       // wave-uniform: the segment whose AND sits in acc
    bool dirty = false;     // wave-uniform: something was ANDed since the last flush
    auto flush = [&]() {
#pragma unroll
        for (int o = LPR; o < kWave; o <<= 1) {
            acc.x &= shfl_xor_u64(acc.x, o);
            if constexpr (!NARROW) acc.y &= shfl_xor_u64(acc.y, o);
        }
        if (lane < LPR && col_live) and_into(q.and_words + (uint64_t)cur * p.rs, acc);
        acc = V16{~0ull, ~0ull};
        dirty = false;
    };

    for (uint64_t tile = w0; tile < w1; ++tile) {
        const uint64_t first = tile * kWave;
        stage_and_hash(img, ridx, p.kmers, p.codes, p.n_kmers, first, p.k, p.n_hash, p.mod, lane);
        const uint32_t n_live = p.n_kmers - first < (uint64_t)kWave ? (uint32_t)(p.n_kmers - first) : (uint32_t)kWave;
        {   // the last s in [0, n_segs) with seg_off[s] <= k-mer: in range whatever seg_off holds
            const uint64_t kmer = first + ((uint32_t)lane < n_live ? (uint32_t)lane : n_live - 1u);
            uint64_t lo = 0, hi = q.n_segs - 1;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo + 1) / 2;
                if (q.seg_off[mid] <= kmer) lo = mid; else hi = mid - 1;
            }
            s_seg[lane] = (uint32_t)lo;
        }
        wave_lds_fence();
        const uint32_t seg_a = wave_uniform(s_seg[0]), seg_b = wave_uniform(s_seg[n_live - 1]);
        const bool one_seg = seg_a == seg_b;
        if (dirty && !(one_seg && seg_a == cur)) flush();
        if (one_seg) cur = seg_a;
#pragma unroll 1
        for (int sub = 0; sub < LPR; ++sub) {
            const int kk = sub * KPW + (lane >> LOG_LPR);
            const bool live = (uint32_t)kk < n_live;
            V16 a{~0ull, ~0ull};   // a dead lane, and a lane past the row's width, leave every AND as it is
            uint32_t zm = ~0u;     // ... and hold no bits of any row
            if (live && col_live) a = gather_and<NARROW, true>(p.mat, p.rs, ridx, kk, col_word, p.n_hash, zm);
            // a row is absent (== all-zero) iff every live lane of its group saw a zero slice for that seed
            uint32_t all_zero = zm;
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) all_zero &= __shfl_xor(all_zero, o, kWave);
            if (live && col == 0 && (all_zero & seeds)) q.missing[s_seg[kk]] = 1;
            if (one_seg) {
                acc.x &= a.x;
                if constexpr (!NARROW) acc.y &= a.y;
            } else if (live && col_live) {
                and_into(q.and_words + (uint64_t)s_seg[kk] * p.rs, a);
            }
        }
        if (one_seg) dirty = true;
    }
    if (dirty) flush();
}

// and_words[s][w] of n_segs x rs words: 0 for an empty segment, for a flagged one and past the last colour
__global__ __launch_bounds__(256) void k_perfect_segments_finish(uint64_t *and_words, const uint8_t *missing, const uint64_t *seg_off,
                                                                 uint64_t n_segs, uint32_t rs, uint32_t n_colors) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_segs * rs) return;
    const uint64_t s = i / rs;
    const uint32_t w = (uint32_t)(i - s * rs);
    uint64_t v = and_words[i];
    if (seg_off[s + 1] == seg_off[s] || missing[s]) v = 0;
    const uint64_t bit0 = 64ull * w;
    if (bit0 >= n_colors) v = 0;
    else if (n_colors - bit0 < 64) v &= (1ull << (n_colors - bit0)) - 1ull;
    and_words[i] = v;
}

size_t perfect_segments_wave_bytes(uint32_t k, uint32_t n_hash) {   // the k-mer image, the row numbers, s_seg
    return ((size_t)kmer_img_bytes(k) + (size_t)kWave * n_hash * 4u + kWave * 4u + 15u) & ~(size_t)15;
}

hipError_t launch_perfect_segments(const PerfectSegmentParams &q, hipStream_t stream) {
    const SearchParams &p = q.s;
    if (p.rs > 128) return hipErrorInvalidValue;   // wide rows: refused by the ABI before it gets here
    const bool narrow = p.rs == 1;
    const int log_lpr = narrow ? 0 : log2u(p.rs / 2);
    const size_t shmem = search_smem_bytes(p);     // c_pad = 0: four waves' staging and nothing else
    const int grid = grid_for(p.n_kmers, p.tiles_per_block);
    if (grid == 0 || q.n_segs == 0) return hipSuccess;
    CID_LAUNCH_BY_LAYOUT(k_perfect_segments, log_lpr, narrow, grid, shmem, stream, q);
}

hipError_t launch_perfect_segments_finish(uint64_t *and_words, const uint8_t *missing, const uint64_t *seg_off, uint64_t n_segs, uint32_t rs,
                                          uint32_t n_colors, hipStream_t stream) {
    const uint64_t n = n_segs * rs;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_perfect_segments_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, and_words, missing, seg_off, n_segs,
                       rs, n_colors);
    return hipGetLastError();
}

}  // namespace cid
