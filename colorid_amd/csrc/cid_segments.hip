// Segmented search for MI355X (gfx950): many queries' k-mers laid end to end, one row of per-colour counters per query
// (src/batch_search_pe.rs:125-164 per segment) and, per segment, cid_search_perfect's "some row is absent" flag
// (src/perfect_search.rs:83-110).  The gather is k_search_count's (cid_gather.hpp: stage_and_hash, gather_and with the zero mask,
// VCount); only where the counts go differs.
//
// Decomposition: tiles are plain runs of 64 consecutive k-mers of the whole array, so a tile MAY span segments.  The tile count then
// depends on n_kmers alone — the device-pointer form needs no scan of the segment lengths and no answer from the device before its launch —
// and every tile starts 16-byte aligned as stage_kmers wants.  Each lane finds the segment of its tile's k-mer by a binary search of
// seg_off (ties, i.e. empty segments, resolve to the last one: the segment that really holds the k-mer).
// A wave owns a contiguous range of tiles and keeps ONE segment's counters: bit-sliced in registers (VCount), drained into a per-wave
// LDS histogram, flushed with one atomicAdd per non-zero colour into hits[s][.] when the wave moves on to another segment and at its
// end.  That is the path of every tile that lies inside one segment: all but two tiles of a segment of a few hundred k-mers and more.
// A tile that holds a segment boundary adds its AND words' bits straight to hits[s][c], one atomic per set bit: at most 64 k-mers
// per boundary, spread over as many rows of `hits` as the tile has segments.  Segments that span waves or workgroups add up through the
// atomics; counts are integers, so the result does not depend on the order.
#include "cid_gather.hpp"

namespace cid {

template <int LOG_LPR, bool NARROW>
__global__ __launch_bounds__(kBlock) void k_search_segments(SegmentParams q) {
    extern __shared__ __align__(16) uint8_t smem[];
    const SearchParams &p = q.s;
    constexpr int LPR = 1 << LOG_LPR;
    constexpr int KPW = kWave / LPR;  // k-mers per sub-pass
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint32_t C = p.n_colors;

    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(smem) + (size_t)wave * p.c_pad;   // [c_pad] this wave's segment (4 waves: 16 * c_pad bytes)
    uint8_t *wbase = smem + 16ull * p.c_pad + (size_t)wave * p.wave_bytes;
    uint32_t *img = reinterpret_cast<uint32_t *>(wbase);
    uint32_t *ridx = reinterpret_cast<uint32_t *>(wbase + kmer_img_bytes(p.k));
    uint32_t *s_seg = ridx + kWave * p.n_hash;   // [64] the segment of every k-mer of the tile

    for (uint32_t c = lane; c < p.c_pad; c += kWave) s_cnt[c] = 0;
    wave_lds_fence();

    const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
    const uint64_t tile0 = (uint64_t)blockIdx.x * p.tiles_per_block;
    const uint64_t tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
    const uint64_t per_wave = (p.tiles_per_block + kBlock / kWave - 1) / (kBlock / kWave);
    const uint64_t w0 = tile0 + (uint64_t)wave * per_wave;
    const uint64_t w1 = w0 + per_wave < tile1 ? w0 + per_wave : tile1;
    const uint32_t col = lane & (LPR - 1);
    const uint32_t col_word = NARROW ? 0u : 2u * col;
    const bool col_live = col_word < p.w64;  // lanes past the row's real width neither load nor count
    const uint32_t seeds = p.n_hash >= 32 ? ~0u : ((1u << p.n_hash) - 1u);

    VCount<kPlanes, NARROW> vc;
    vc.clear();
    uint32_t cur = 0;      // wave-uniform: the segment whose counts sit in vc / s_cnt
    bool dirty = false;    // wave-uniform: something was counted since the last flush
    auto flush = [&]() {
        vc.drain(s_cnt, col_word);
        wave_lds_fence();
        uint32_t *row = q.hits + (uint64_t)cur * C;
        for (uint32_t c = lane; c < C; c += kWave) {
            const uint32_t h = s_cnt[c];
            if (h) { atomicAdd(&row[c], h); s_cnt[c] = 0; }
        }
        wave_lds_fence();
        dirty = false;
    };
    auto add_bits = [&](uint32_t *row, uint32_t base, uint64_t w) {   // a boundary tile: one atomic per set bit
        while (w) {
            const uint32_t c = base + (uint32_t)__builtin_ctzll(w);
            if (c < C) atomicAdd(&row[c], 1u);
            w &= w - 1;
        }
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
            V16 a{0, 0};
            uint32_t zm = ~0u;   // a dead lane holds no bits of any row
            if (live && col_live) a = gather_and<NARROW, true>(p.mat, p.rs, ridx, kk, col_word, p.n_hash, zm);
            if constexpr (NARROW) a.y = 0;
            // a row is absent (== all-zero) iff every live lane of its group saw a zero slice for that seed
            uint32_t all_zero = zm;
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) all_zero &= __shfl_xor(all_zero, o, kWave);
            if (live && col == 0 && q.missing && (all_zero & seeds)) q.missing[s_seg[kk]] = 1;
            if (one_seg) {
                vc.add(a);  // hits[c] += bit c, for this lane's colours
                if (vc.full()) vc.drain(s_cnt, col_word);
            } else if (live) {
                uint32_t *row = q.hits + (uint64_t)s_seg[kk] * C;
                add_bits(row, col_word * 64u, a.x);
                if constexpr (!NARROW) add_bits(row, col_word * 64u + 64u, a.y);
            }
        }
        if (one_seg) dirty = true;
    }
    if (dirty) flush();
}

hipError_t launch_search_segments(const SegmentParams &q, hipStream_t stream) {
    const SearchParams &p = q.s;
    if (p.rs > 128) return hipErrorInvalidValue;   // wide rows: refused by the ABI before it gets here
    const bool narrow = p.rs == 1;
    const int log_lpr = narrow ? 0 : log2u(p.rs / 2);
    const size_t shmem = search_smem_bytes(p);
    const int grid = grid_for(p.n_kmers, p.tiles_per_block);
    if (grid == 0 || q.n_segs == 0) return hipSuccess;
    CID_LAUNCH_BY_LAYOUT(k_search_segments, log_lpr, narrow, grid, shmem, stream, q);
}

}  // namespace cid
