// Greedy cover for MI355X (gfx950): the accessions that explain a query, one per round (include/colorid_hip.h: cid_search_gather).
// Not to be confused with cid_gather.hpp, which gathers ROWS; this file gathers ACCESSIONS, as `sourmash gather` does.
//
// Input is k_cover_rows' matrix (cid_cover.hip): rows[k][rs], the AND words of query k-mer k, and the k-mers' multiplicities.  All
// arithmetic is integer sums and the pick is a total order, so the result does not depend on how the grid splits the work.
//
//   k_gather_init     alive[t] = which rows of tile t (64 consecutive rows) have a colour at all; n_hit = their number.  Rows without a
//                     colour are live for ever (they count in live_before) but no round can touch them: they are left out of the masks.
//   k_gather_fold     one wave per (range of tiles, 64-colour word j): lane l loads word j of row 64t + l for the rows a mask selects, the
//                     wave transposes the 64 x 64 bit block (transpose_bits64) and lane c, which then holds the 64 row bits of colour
//                     64j + c, popcounts them into a register; one atomic per colour at the wave's end.  Tiles whose mask is zero cost
//                     one wave-uniform load.  TOTALS: the mask is alive[], the sums go to total[] and — each row bit weighed with its
//                     k-mer's multiplicity, fetched from the row's lane — total_weight[].  Otherwise: the mask is removed[], and the
//                     counts are SUBTRACTED from new[]: a round costs what it removes, not rows x colours.
//   k_gather_pick     one workgroup: arg-max of new[] (largest count, then lowest colour); appends the row or sets the stop flag.
//   k_gather_mark     reads word pick / 64 of every row that is still alive: removed[t] = the alive rows with the pick's bit, which leave
//                     alive[t]; the sum of their multiplicities is the row's new_weight.
// A round is pick (the host reads 16 bytes: stop?) -> mark -> fold.  new[pick] is zero afterwards, so a colour is picked once.
#include "../../include/colorid_hip.h"
#include "cid_gather.hpp"

namespace cid {

static_assert(sizeof(cid_gather_row) == 48, "cid_gather_row is part of the ABI");

namespace {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, kWave), hi = __shfl_xor((uint32_t)(v >> 32), o, kWave);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// this wave's tiles [t0, t1) of the n_tiles, tiles_per_wave consecutive ones per wave number g
__device__ __forceinline__ void wave_tiles(const GatherParams &p, uint64_t g, uint64_t &t0, uint64_t &t1) {
    const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
    t0 = g * p.tiles_per_wave;
    t1 = t0 + p.tiles_per_wave < n_tiles ? t0 + p.tiles_per_wave : n_tiles;
}

__device__ __forceinline__ uint64_t this_wave() { return wave_uniform((uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6)); }

}  // namespace

__global__ __launch_bounds__(kBlock) void k_gather_init(GatherParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    uint64_t t0, t1;
    wave_tiles(p, this_wave(), t0, t1);
    uint32_t n = 0;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t row = t * kWave + lane;
        uint64_t any = 0;
        if (row < p.n_kmers)
            for (uint32_t j = 0; j < p.w64; ++j) any |= p.rows[row * p.rs + j];
        const uint64_t m = __ballot(any != 0);
        if (lane == 0) { p.alive[t] = m; p.removed[t] = 0; }
        n += (uint32_t)__popcll(m);
    }
    if (lane == 0 && n) atomicAdd(&p.round->n_hit, (unsigned long long)n);
}

template <bool TOTALS>
__global__ __launch_bounds__(kBlock) void k_gather_fold(GatherParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t g = this_wave();
    const uint32_t j = (uint32_t)(g % p.w64);
    uint64_t t0, t1;
    wave_tiles(p, g / p.w64, t0, t1);   // past the last range: t0 >= t1, nothing to do
    if constexpr (!TOTALS) {
        if (wave_uniform(p.round->stop)) return;
    }
    const uint64_t *mask = TOTALS ? p.alive : p.removed;
    uint64_t cnt = 0, wsum = 0;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t m = wave_uniform(mask[t]);   // only rows below n_kmers are ever set in a mask
        if (m == 0) continue;
        const uint64_t row = t * kWave + lane;
        const bool sel = (m >> lane) & 1ull;
        const uint64_t x = transpose_bits64(sel ? p.rows[row * p.rs + j] : 0ull, lane);
        cnt += (uint64_t)__popcll(x);
        if constexpr (TOTALS) {
            if (p.freq) {
                const uint32_t f = sel ? p.freq[row] : 0u;
                for (uint64_t mm = m; mm; mm &= mm - 1) {   // wave-uniform: the selected rows, one after the other
                    const int i = __builtin_ctzll(mm);
                    const uint32_t fi = (uint32_t)__builtin_amdgcn_readlane((int)f, i);
                    wsum += ((x >> i) & 1ull) ? fi : 0u;
                }
            }
        }
    }
    const uint32_t c = j * 64u + lane;
    if (c >= p.n_colors || cnt == 0) return;
    if constexpr (TOTALS) {
        atomicAdd(&p.total[c], (unsigned long long)cnt);
        atomicAdd(&p.total_weight[c], (unsigned long long)(p.freq ? wsum : cnt));
    } else {
        atomicAdd(&p.cnt_new[c], (unsigned long long)(0 - cnt));   // subtract: the rows were counted in when they were alive
    }
}

__global__ __launch_bounds__(kBlock) void k_gather_mark(GatherParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    const GatherRound r = *p.round;   // wave-uniform
    const uint32_t c = wave_uniform(r.colour);
    const uint64_t slot = wave_uniform(r.n_out) - 1;   // the row k_gather_pick has just appended
    if (wave_uniform(r.stop) || c >= p.n_colors || slot >= p.max_rows) return;
    const uint32_t word = c >> 6, bit = c & 63u;
    uint64_t t0, t1;
    wave_tiles(p, this_wave(), t0, t1);
    uint64_t wsum = 0;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t a = wave_uniform(p.alive[t]);
        uint64_t m = 0;
        if (a) {
            const uint64_t row = t * kWave + lane;
            const bool sel = (a >> lane) & 1ull;
            const bool hit = sel && ((p.rows[row * p.rs + word] >> bit) & 1ull);
            m = __ballot(hit);
            if (hit) wsum += p.freq ? p.freq[row] : 1u;
        }
        if (lane == 0) {
            p.removed[t] = m;
            if (m) p.alive[t] = a & ~m;
        }
    }
    wsum = wave_sum_u64(wsum);
    if (lane == 0 && wsum) atomicAdd(reinterpret_cast<unsigned long long *>(&static_cast<cid_gather_row *>(p.out)[slot].new_weight), (unsigned long long)wsum);
}

__global__ __launch_bounds__(kBlock) void k_gather_pick(GatherParams p) {
    __shared__ unsigned long long s_v[kBlock / kWave];
    __shared__ uint32_t s_c[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned long long v = 0;
    uint32_t c = 0xFFFFFFFFu;   // no colour: loses every tie
    for (uint32_t i = threadIdx.x; i < p.n_colors; i += kBlock) {
        const unsigned long long x = p.cnt_new[i];
        if (c == 0xFFFFFFFFu || x > v) { v = x; c = i; }   // ascending i: an equal count keeps the lower colour
    }
    auto better = [](unsigned long long va, uint32_t ca, unsigned long long vb, uint32_t cb) { return va > vb || (va == vb && ca < cb); };
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, kWave), hi = __shfl_xor((uint32_t)(v >> 32), o, kWave), oc = __shfl_xor(c, o, kWave);
        const unsigned long long ov = ((unsigned long long)hi << 32) | lo;
        if (better(ov, oc, v, c)) { v = ov; c = oc; }
    }
    if (lane == 0) { s_v[wave] = v; s_c[wave] = c; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kBlock / kWave; ++w)
        if (better(s_v[w], s_c[w], v, c)) { v = s_v[w]; c = s_c[w]; }
    GatherRound r = *p.round;
    if (r.n_out >= p.max_rows || v < p.min_new || c >= p.n_colors) {
        p.round->stop = 1u;
        return;
    }
    cid_gather_row row;
    row.colour = c; row.reserved = 0;
    row.new_kmers = v; row.new_weight = 0;   // k_gather_mark adds the weights up
    row.total_kmers = p.total[c]; row.total_weight = p.total_weight[c];
    row.live_before = r.live;
    static_cast<cid_gather_row *>(p.out)[r.n_out] = row;
    r.colour = c; r.n_out += 1; r.live -= v;
    *p.round = r;
}

namespace {
// `waves` waves, four a workgroup
template <class K>
hipError_t launch_waves(K kernel, uint64_t waves, const GatherParams &p, hipStream_t stream) {
    if (waves == 0) return hipSuccess;
    const uint64_t grid = (waves + kBlock / kWave - 1) / (kBlock / kWave);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
}
uint64_t tile_ranges(const GatherParams &p) {
    const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
    return (n_tiles + p.tiles_per_wave - 1) / p.tiles_per_wave;
}
}  // namespace

hipError_t launch_gather_init(const GatherParams &p, hipStream_t stream) { return launch_waves(k_gather_init, tile_ranges(p), p, stream); }

hipError_t launch_gather_totals(const GatherParams &p, hipStream_t stream) {
    return launch_waves(k_gather_fold<true>, tile_ranges(p) * p.w64, p, stream);
}

hipError_t launch_gather_pick(const GatherParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(k_gather_pick, dim3(1), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_gather_round(const GatherParams &p, hipStream_t stream) {
    hipError_t e = launch_waves(k_gather_mark, tile_ranges(p), p, stream);
    if (e != hipSuccess) return e;
    return launch_waves(k_gather_fold<false>, tile_ranges(p) * p.w64, p, stream);
}

}  // namespace cid
