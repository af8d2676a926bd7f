// Segmented perfect search for MI355X (gfx950): many queries' k-mers laid end to end, per query the AND of all its k-mers' rows
// (src/perfect_search.rs:83-110 per segment) and cid_search_perfect's "some row is absent" flag — `search -s -m`, where every record of a
// scheme's multi-FASTA is an allele and the answer per record is C bits, not C counters.
//
// Decomposition, staging, gather and the walk of a wave through its segments are cid_segwalk.hpp's, shared with k_search_segments.  This
// file is where the result goes.  A wave keeps ONE segment's running AND in registers: every lane its own column words, preset to all
// ones; a dead lane contributes all ones.  On a flush the 64 / LPR k-mer groups are reduced with __shfl_xor and the lanes of group 0
// atomicAnd their one or two u64 words into and_words[seg][.]: no LDS histogram, no counters.  A tile that holds a segment boundary ANDs
// each live lane's words straight into the row of that lane's own segment: at most two atomics per lane and sub-pass (64 * LPR lane
// visits per tile), however many colours hit.  AND is associative and idempotent, so segments that span waves, workgroups or launches
// need nothing but the atomics, and the result is bit-exact in any order.
//
// The caller presets and_words to all ones and the flags to 0; k_perfect_segments_finish then applies the contract: zero words for an
// empty segment, for a flagged one (as cid_search_perfect zeroes them), and for the bits at and above n_colors.
#include "cid_segwalk.hpp"

namespace cid {

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, kWave), hi = __shfl_xor((uint32_t)(v >> 32), o, kWave);
    return ((uint64_t)hi << 32) | lo;
}

template <int LOG_LPR, bool NARROW>
struct AndSink {   // walk_segment_tiles' sink
    uint64_t *and_words;   // [n_segs][rs]
    uint32_t rs, col_word;
    bool group0;           // the lanes that store a flush: k-mer group 0, within the row's width
    V16 acc;               // this lane's column words of the segment, ANDed over the k-mers this lane has seen

    __device__ __forceinline__ V16 dead() const { return V16{~0ull, ~0ull}; }   // leaves every AND as it is
    __device__ __forceinline__ void own(V16 a) {
        acc.x &= a.x;
        if constexpr (!NARROW) acc.y &= a.y;
    }
    __device__ __forceinline__ void and_into(uint32_t seg, V16 a) {   // this lane's words into the segment's row; all ones change nothing: no atomic
        uint64_t *row = and_words + (uint64_t)seg * rs;
        if (a.x != ~0ull) atomicAnd(reinterpret_cast<unsigned long long *>(&row[col_word]), (unsigned long long)a.x);
        if constexpr (!NARROW)
            if (a.y != ~0ull) atomicAnd(reinterpret_cast<unsigned long long *>(&row[col_word + 1]), (unsigned long long)a.y);
    }
    __device__ __forceinline__ void stray(uint32_t seg, V16 a) { and_into(seg, a); }
    __device__ __forceinline__ void flush(uint32_t seg) {
#pragma unroll
        for (int o = 1 << LOG_LPR; o < kWave; o <<= 1) {
            acc.x &= shfl_xor_u64(acc.x, o);
            if constexpr (!NARROW) acc.y &= shfl_xor_u64(acc.y, o);
        }
        if (group0) and_into(seg, acc);
        acc = dead();
    }
};

template <int LOG_LPR, bool NARROW>
__global__ __launch_bounds__(kBlock) void k_perfect_segments(PerfectSegmentParams q) {
    extern __shared__ __align__(16) uint8_t smem[];
    const SearchParams &p = q.s;
    const TileWave<LOG_LPR, NARROW> w(p, smem);
    AndSink<LOG_LPR, NARROW> sink{q.and_words, p.rs, w.col_word, w.lane < w.LPR && w.col_live, V16{~0ull, ~0ull}};
    walk_segment_tiles(p, q.seg_off, q.n_segs, q.missing, w, sink);
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
    CID_LAUNCH_TILES(k_perfect_segments, q.s, q.n_segs == 0, stream, q);   // c_pad = 0: four waves' staging and nothing else
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
