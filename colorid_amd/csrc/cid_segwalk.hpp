// The tile walk of the segmented search kernels (gfx950, wave64), written once: what a wave of a tile kernel knows about itself
// (TileWave: k_search_segments, k_perfect_segments, k_cover_rows, k_search_perfect), and the loop that takes a wave through its tiles
// segment by segment (walk_segment_tiles: the first two).  No kernels here; DESIGN.md §4 "Segmented search".
//
// Decomposition: tiles are plain runs of 64 consecutive k-mers of the whole array, so a tile MAY span segments.  The tile count then
// depends on n_kmers alone — the device-pointer form needs no scan of the segment lengths and no answer from the device before its launch —
// and every tile starts 16-byte aligned as stage_kmers wants.  Each lane finds the segment of its tile's k-mer by a binary search of
// seg_off (segment_of, cid_segplan.hpp: ties, i.e. empty segments, resolve to the last one, the segment that really holds the k-mer).
// A wave owns a contiguous range of tiles and keeps ONE segment's running result in a sink: it flushes the sink into that segment's row
// when it moves on to another segment, and at its end.  That is the path of every tile that lies inside one segment (`own`): all but two
// tiles of a segment of a few hundred k-mers and more.  In a tile that holds a segment boundary every live lane sends its AND words
// straight to the row of its own k-mer's segment (`stray`): at most 64 k-mers per boundary.  Segments that span waves, workgroups or
// launches combine through the sinks' atomics, which are order-independent (integer sums; AND).
#pragma once
#include "cid_gather.hpp"
#include "cid_segplan.hpp"

namespace cid {

// AND over the LPR adjacent lanes that share a row: group_sum's counterpart (cid_gather.hpp).  Every lane of the wave must call it —
// before any divergent test of its result, never inside a short-circuit condition.
template <int LOG_LPR>
__device__ __forceinline__ uint32_t group_and(uint32_t v) {
#pragma unroll
    for (int o = 1; o < (1 << LOG_LPR); o <<= 1) v &= __shfl_xor(v, o, kWave);
    return v;
}

// One wave of a tile kernel: its staging area in LDS, the tiles of its workgroup and its own share of them, its lanes' place in a row.
// LPR = 2^LOG_LPR adjacent lanes cover one row with 16 bytes each (NARROW: one lane, 8 bytes), so a sub-pass covers 64 / LPR k-mers.
template <int LOG_LPR, bool NARROW>
struct TileWave {
    static constexpr int LPR = 1 << LOG_LPR;
    static constexpr int KPW = kWave / LPR;   // k-mers per sub-pass
    int lane, wave;
    uint32_t *img, *ridx;     // the k-mer image and the hash rows (stage_and_hash)
    uint32_t *past_rows;      // what the launch's wave_bytes leave behind the hash rows, if anything
    uint64_t tile0, tile1;    // the workgroup's tiles
    uint64_t w0, w1;          // this wave's contiguous share of them
    uint32_t col, col_word;   // this lane's place among the LPR lanes of a row, and its first u64 word of the row
    bool col_live;            // lanes past the row's real width neither load nor contribute

    __device__ __forceinline__ TileWave(const SearchParams &p, uint8_t *smem) {
        lane = threadIdx.x & (kWave - 1);
        wave = threadIdx.x >> 6;
        uint8_t *wbase = smem + 16ull * p.c_pad + (size_t)wave * p.wave_bytes;   // behind the workgroup's 16 * c_pad bytes, if it has any
        img = reinterpret_cast<uint32_t *>(wbase);
        ridx = reinterpret_cast<uint32_t *>(wbase + kmer_img_bytes(p.k));
        past_rows = ridx + kWave * p.n_hash;
        const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
        tile0 = (uint64_t)blockIdx.x * p.tiles_per_block;
        tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
        const uint64_t per_wave = (p.tiles_per_block + kBlock / kWave - 1) / (kBlock / kWave);
        w0 = tile0 + (uint64_t)wave * per_wave;
        w1 = w0 + per_wave < tile1 ? w0 + per_wave : tile1;
        col = lane & (LPR - 1);
        col_word = NARROW ? 0u : 2u * col;
        col_live = col_word < p.w64;
    }
    __device__ __forceinline__ int kk(int sub) const { return sub * KPW + (lane >> LOG_LPR); }   // this lane's k-mer of the tile in sub-pass `sub`
};

// The wave's tiles w.w0 .. w.w1, each staged, hashed and gathered (gather_and with the zero mask), its AND words handed to `sink`; sets
// missing[s] (unless null) for every segment s with a k-mer one of whose rows is absent.  LDS: 64 u32 at w.past_rows, the segment of
// every k-mer of the tile.  A sink keeps one segment's running result and supplies
//   V16 dead()                 what a dead lane — past the last k-mer, or past the row's width — contributes
//   void own(V16 a)            a tile inside one segment: all lanes call it, for the segment the next flush will name
//   void stray(seg, V16 a)     a boundary tile: only lanes that are live, in k-mer and in column, call it, each for its own k-mer's segment
//   void flush(seg)            the running result goes to segment `seg` and starts afresh; all lanes call it
// The walk owns which segment that is (`cur`) and whether anything went into the sink since the last flush (`dirty`); both are wave-uniform.
template <int LOG_LPR, bool NARROW, class Sink>
__device__ __forceinline__ void walk_segment_tiles(const SearchParams &p, const uint64_t *seg_off, uint64_t n_segs, uint8_t *missing,
                                                   const TileWave<LOG_LPR, NARROW> &w, Sink &sink) {
    constexpr int LPR = 1 << LOG_LPR;
    uint32_t *s_seg = w.past_rows;
    const uint32_t seeds = p.n_hash >= 32 ? ~0u : ((1u << p.n_hash) - 1u);
    uint32_t cur = 0;
    bool dirty = false;
    for (uint64_t tile = w.w0; tile < w.w1; ++tile) {
        const uint64_t first = tile * kWave;
        stage_and_hash(w.img, w.ridx, p.kmers, p.codes, p.n_kmers, first, p.k, p.n_hash, p.mod, w.lane);
        const uint32_t n_live = p.n_kmers - first < (uint64_t)kWave ? (uint32_t)(p.n_kmers - first) : (uint32_t)kWave;
        s_seg[w.lane] = (uint32_t)segment_of(seg_off, n_segs, first + ((uint32_t)w.lane < n_live ? (uint32_t)w.lane : n_live - 1u));
        wave_lds_fence();
        const uint32_t seg_a = wave_uniform(s_seg[0]), seg_b = wave_uniform(s_seg[n_live - 1]);
        const bool one_seg = seg_a == seg_b;
        if (dirty && !(one_seg && seg_a == cur)) { sink.flush(cur); dirty = false; }
        if (one_seg) cur = seg_a;
#pragma unroll 1
        for (int sub = 0; sub < LPR; ++sub) {
            const int kk = w.kk(sub);
            const bool live = (uint32_t)kk < n_live;
            V16 a = sink.dead();
            uint32_t zm = ~0u;   // a dead lane holds no bits of any row
            if (live && w.col_live) a = gather_and<NARROW, true>(p.mat, p.rs, w.ridx, kk, w.col_word, p.n_hash, zm);
            // a row is absent (== all-zero) iff every live lane of its group saw a zero slice for that seed
            const uint32_t all_zero = group_and<LOG_LPR>(zm);
            if (live && w.col == 0 && missing && (all_zero & seeds)) missing[s_seg[kk]] = 1;
            if (one_seg) sink.own(a);
            else if (live && w.col_live) sink.stray(s_seg[kk], a);
        }
        if (one_seg) dirty = true;
    }
    if (dirty) sink.flush(cur);
}

}  // namespace cid
