// Segmented search for MI355X (gfx950): many queries' k-mers laid end to end, one row of per-colour counters per query
// (src/batch_search_pe.rs:125-164 per segment) and, per segment, cid_search_perfect's "some row is absent" flag
// (src/perfect_search.rs:83-110).  The gather is k_search_count's (cid_gather.hpp: stage_and_hash, gather_and with the zero mask,
// VCount); the decomposition into tiles and the walk of a wave through its segments are cid_segwalk.hpp's.  This file is where the
// counts go: a wave keeps ONE segment's counters bit-sliced in registers (VCount), drained into a per-wave LDS histogram, flushed with
// one atomicAdd per non-zero colour into hits[s][.].  A tile that holds a segment boundary adds its AND words' bits straight to
// hits[s][c], one atomic per set bit, spread over as many rows of `hits` as the tile has segments.  Counts are integers, so the result
// does not depend on the order.
#include "cid_segwalk.hpp"

namespace cid {

template <bool NARROW>
struct CountSink {   // walk_segment_tiles' sink
    uint32_t *hits;      // [n_segs][C]
    uint32_t C;
    uint32_t *s_cnt;     // [c_pad] this wave's segment, in LDS
    uint32_t col_word;
    int lane;
    VCount<kPlanes, NARROW> vc;

    __device__ __forceinline__ V16 dead() const { return V16{0, 0}; }
    __device__ __forceinline__ void own(V16 a) {
        if constexpr (NARROW) a.y = 0;
        vc.add(a);  // hits[c] += bit c, for this lane's colours
        if (vc.full()) vc.drain(s_cnt, col_word);
    }
    __device__ __forceinline__ void add_bits(uint32_t *row, uint32_t base, uint64_t w) {   // one atomic per set bit
        while (w) {
            const uint32_t c = base + (uint32_t)__builtin_ctzll(w);
            if (c < C) atomicAdd(&row[c], 1u);
            w &= w - 1;
        }
    }
    __device__ __forceinline__ void stray(uint32_t seg, V16 a) {
        uint32_t *row = hits + (uint64_t)seg * C;
        add_bits(row, col_word * 64u, a.x);
        if constexpr (!NARROW) add_bits(row, col_word * 64u + 64u, a.y);
    }
    __device__ __forceinline__ void flush(uint32_t seg) {
        vc.drain(s_cnt, col_word);
        wave_lds_fence();
        uint32_t *row = hits + (uint64_t)seg * C;
        for (uint32_t c = lane; c < C; c += kWave) {
            const uint32_t h = s_cnt[c];
            if (h) { atomicAdd(&row[c], h); s_cnt[c] = 0; }
        }
        wave_lds_fence();
    }
};

template <int LOG_LPR, bool NARROW>
__global__ __launch_bounds__(kBlock) void k_search_segments(SegmentParams q) {
    extern __shared__ __align__(16) uint8_t smem[];
    const SearchParams &p = q.s;
    const TileWave<LOG_LPR, NARROW> w(p, smem);
    CountSink<NARROW> sink{q.hits, p.n_colors, reinterpret_cast<uint32_t *>(smem) + (size_t)w.wave * p.c_pad, w.col_word, w.lane, {}};   // (4 waves: 16 * c_pad bytes)
    for (uint32_t c = w.lane; c < p.c_pad; c += kWave) sink.s_cnt[c] = 0;
    wave_lds_fence();
    sink.vc.clear();
    walk_segment_tiles(p, q.seg_off, q.n_segs, q.missing, w, sink);
}

hipError_t launch_search_segments(const SegmentParams &q, hipStream_t stream) {
    CID_LAUNCH_TILES(k_search_segments, q.s, q.n_segs == 0, stream, q);
}

}  // namespace cid
