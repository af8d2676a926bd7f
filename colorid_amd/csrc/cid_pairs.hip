// `colorid compare` kernels for MI355X (gfx950): the Gram matrix of an index's bit matrix, shared[i][j] = popcount(column i & column j),
// from the rows as a .bxi/.mxi file holds them or from a resident index (cid_pairs_*).  Integer sums only: exact, whatever the schedule.
#include <algorithm>

#include "cid_kernels.hpp"
#include "cid_records.hpp"

namespace cid {

// The records of one upload chunk against the file's shape, one thread per record: err[0] |= check_record's bits (cid_records.hpp), as
// the put kernels do.  Run before k_pairs, so a refused chunk adds nothing.
__global__ void k_pairs_check(const uint32_t *rec32, uint32_t w32_rec, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors,
                              uint32_t tail_mask, uint32_t *err) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_records) return;
    const uint32_t *rec = rec32 + r * record_words(w32_rec);
    const uint32_t e = check_record(rec, record_row(rec), w32_rec, n_colors, bloom_size, tail_mask);
    if (e) atomicOr(err, e);
}

// Block pair number -> (I, J), I <= J < nb, pairs of one I consecutive: pair_base(I) = I*nb - I*(I-1)/2.
__device__ __forceinline__ uint64_t pair_base(uint64_t I, uint64_t nb) { return I * nb - I * (I - 1) / 2; }
__device__ __forceinline__ void pair_of(uint64_t pair, uint32_t nb, uint32_t &I, uint32_t &J) {
    const double t = 2.0 * nb + 1.0;
    int64_t i = (int64_t)((t - sqrt(t * t - 8.0 * (double)pair)) * 0.5);   // the root of pair_base(i) = pair, then set right
    if (i < 0) i = 0;
    if (i >= nb) i = nb - 1;
    while (i > 0 && pair_base((uint64_t)i, nb) > pair) --i;
    while ((uint64_t)i + 1 < nb && pair_base((uint64_t)i + 1, nb) <= pair) ++i;
    I = (uint32_t)i;
    J = I + (uint32_t)(pair - pair_base((uint64_t)i, nb));
}

// The 64 x 64 bit tile whose row r is lane r's word, transposed: lane l returns column l (bit r = bit l of lane r's word).  Six
// butterfly stages, widths 32 .. 1: the lanes l and l ^ w swap the two off-diagonal w x w blocks of every 2w x 2w block.
__device__ __forceinline__ unsigned long long transpose64(unsigned long long x, uint32_t lane) {
    unsigned long long m = 0x00000000FFFFFFFFull;   // the bit positions whose bit w is clear
#pragma unroll
    for (int w = 32; w; w >>= 1) {
        const unsigned long long y = __shfl_xor(x, w);
        x = (lane & (uint32_t)w) ? ((x & ~m) | ((y >> w) & m)) : ((x & m) | ((y & m) << w));
        m ^= m << (w >> 1);
    }
    return x;
}

// The 64 colours of a block are one 64-bit word of a row (two u32 words; the second may lie past an odd w32: zero then).  A wave owns
// one block pair (I, J) over the row tiles [tile0, tile1) of its workgroup; the four waves of a workgroup take four consecutive pairs of
// the SAME tiles, so the rows a workgroup reads come to its CU once.  Per tile of 64 rows lane r holds row r's words of I and of J.  The
// tile's J words are transposed across the lanes (transpose64): lane l holds column l of J over the tile's 64 rows, `mine`.
// 64 ballots over the I word give the columns of I one after the other, wave-uniform: acc[b] += popcount(mine & column b of I) — two
// ANDs, two v_bcnt and an add.  After the tiles acc[b] of lane l is shared[64 I + b][64 J + l]: each of the 64 flushes is one
// wave instruction over 512 contiguous bytes of counters (64-bit vector atomics; the memory side wants contiguous adds), only for
// i <= j < C — the host mirrors the triangle.  Rows past n_rows load as zero and add nothing; so do the all-zero rows of a resident index.
// BOUND: a tile adds at most 64 to a counter, a workgroup sees at most kPairsMaxTiles = 2^16 tiles (launch_pairs), so acc <= 2^22 < 2^32.
__global__ __launch_bounds__(kBlock) void k_pairs(PairsParams p) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint64_t pair = (uint64_t)(blockIdx.x % p.n_pair_groups) * (kBlock / kWave) + wave;
    if (pair >= p.n_pairs) return;   // wave-uniform: the last group of pairs may be short
    uint32_t I, J;
    pair_of(pair, p.n_blocks, I, J);
    const uint64_t n_tiles = (p.n_rows + kWave - 1) / kWave;
    const uint64_t tile0 = ((uint64_t)(blockIdx.x / p.n_pair_groups) + p.chunk0) * p.tiles_per_block;
    const uint64_t tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
    const bool i_hi = 2u * I + 1u < p.w32, j_hi = 2u * J + 1u < p.w32;
    uint32_t ilo = 0, ihi = 0, jlo = 0, jhi = 0;
    auto load = [&](uint64_t tile) {
        const uint64_t row = tile * kWave + lane;
        ilo = ihi = jlo = jhi = 0;
        if (row < p.n_rows) {
            const uint32_t *w = p.rows + row * p.stride + p.off;
            ilo = w[2u * I];
            if (i_hi) ihi = w[2u * I + 1u];
            jlo = w[2u * J];
            if (j_hi) jhi = w[2u * J + 1u];
        }
    };
    uint32_t acc[64];
#pragma unroll
    for (int b = 0; b < 64; ++b) acc[b] = 0;
    if (tile0 < tile1) load(tile0);
    for (uint64_t tile = tile0; tile < tile1; ++tile) {
        const uint32_t ci_lo = ilo, ci_hi = ihi, cj_lo = jlo, cj_hi = jhi;
        if (tile + 1 < tile1) load(tile + 1);   // the next tile's words are on their way while this one is counted
        const unsigned long long mine = transpose64((unsigned long long)cj_lo | ((unsigned long long)cj_hi << 32), lane);
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            const unsigned long long col = __ballot(((b < 32 ? ci_lo >> b : ci_hi >> (b - 32)) & 1u) != 0);
            acc[b] += (uint32_t)__popcll(mine & col);
        }
    }
    const uint64_t j = 64ull * J + lane;
#pragma unroll
    for (int b = 0; b < 64; ++b) {
        const uint64_t i = 64ull * I + (uint32_t)b;
        if (acc[b] && i <= j && j < p.n_colors) atomicAdd(&p.shared[i * p.n_colors + j], (unsigned long long)acc[b]);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

hipError_t launch_pairs_check(const uint32_t *d_records, uint32_t w32_rec, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors,
                              uint32_t *d_err, hipStream_t stream) {
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pairs_check, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, stream, d_records, w32_rec, n_records, bloom_size,
                       n_colors, tail_mask(n_colors), d_err);
    return hipGetLastError();
}

// Workgroups = groups of four block pairs x row chunks.  The chunks are sized so that about four workgroups per CU exist (each flushes
// 4 x 4096 counters: few enough that the atomics stay far below the counting) and never hold more than kPairsMaxTiles tiles — the bound
// of k_pairs' 32-bit accumulators.  A launch takes at most 2^30 workgroups; a wider grid goes out in several launches.
constexpr uint64_t kPairsMaxTiles = 1ull << 16;
static_assert(kPairsMaxTiles * 64ull < (1ull << 32), "k_pairs accumulates a workgroup's tiles in 32 bits");

hipError_t launch_pairs(PairsParams p, int n_cu, hipStream_t stream) {
    const uint64_t n_tiles = (p.n_rows + kWave - 1) / kWave;
    if (n_tiles == 0 || p.n_colors == 0) return hipSuccess;
    p.n_blocks = (p.n_colors + 63u) / 64u;
    p.n_pairs = (uint64_t)p.n_blocks * (p.n_blocks + 1ull) / 2ull;
    const uint64_t npg = (p.n_pairs + (kBlock / kWave) - 1) / (kBlock / kWave);
    if (npg >= (1ull << 30)) return hipErrorInvalidValue;   // (n_colors <= 2^20: at most 2^25 groups)
    p.n_pair_groups = (uint32_t)npg;
    const uint64_t target = (uint64_t)(n_cu > 0 ? n_cu : 256) * 4;
    uint64_t chunks = std::min<uint64_t>(n_tiles, std::max<uint64_t>(1, (target + npg - 1) / npg));
    uint64_t tpb = std::min<uint64_t>((n_tiles + chunks - 1) / chunks, kPairsMaxTiles);
    chunks = (n_tiles + tpb - 1) / tpb;
    p.tiles_per_block = (uint32_t)tpb;
    const uint64_t chunks_per_launch = std::max<uint64_t>(1, (1ull << 30) / npg);
    for (uint64_t c0 = 0; c0 < chunks; c0 += chunks_per_launch) {
        p.chunk0 = c0;
        const uint64_t nc = std::min<uint64_t>(chunks_per_launch, chunks - c0);
        hipLaunchKernelGGL(k_pairs, dim3((unsigned)(npg * nc)), dim3(kBlock), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace cid
