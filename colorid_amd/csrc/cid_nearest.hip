// Nearest-allele reduction for MI355X (gfx950): from k_search_segments' counters hits[s][c] to, per (group of segments, colour), the
// segment with the largest share hits / length — `search -s -m --alleles --nearest`, where a group is the alleles of one locus and the
// answer says which known allele an accession's uncalled locus is closest to (include/colorid_hip.h: cid_search_nearest_segments).
//
// Order.  A candidate is a segment with length > 0 and hits > 0.  a beats b iff hits_a * len_b > hits_b * len_a (both factors below 2^32:
// exact in u64, no float) or the products are equal and a is the earlier segment.  This is a total order, so the reduction may be split
// anywhere: over the waves of a workgroup here, over slices of segments by the host form (the cell in `out` is merged into, and holds the
// earlier segments' winner).  Walking segments in ascending order and replacing only on a strictly greater share keeps the lowest index.
//
// Decomposition.  A workgroup of four waves owns kNearestGroups = 4 consecutive groups x 64 consecutive colours, and with them their cells of
// `out`: no other workgroup of the launch touches them, so there are no atomics.  Lane l of every wave is colour 64 * blockIdx.y + l: a
// segment's counters are read as one coalesced 256-byte row piece per wave.  The workgroup's segments — those of its four groups, clipped
// to the launch's range — are cut into four equal contiguous runs, one per wave, whatever the groups' sizes: a group of 10 000 alleles
// is walked 2 500 segments to a wave, four one-allele groups take one segment per wave, and neither case leaves waves without work.  A wave
// keeps one group's running best in four registers; when its run crosses into the next group it parks the finished group's partial in
// LDS (part[wave][group][lane], 16 KiB).  After one barrier wave g merges the cell of local group g with the four waves' partials in wave
// order (= ascending segments) and stores it, 16 bytes per lane, 1 KiB per wave.  The segment loop has no dependence between
// iterations but the compare, so the loads of several segments are in flight (sixteen rows are loaded, then compared).
//
// Every index read from group_off is clamped to the launch's segment range [s_lo, s_hi] before it is used, and a segment is assigned only
// to one of the workgroup's own four groups: whatever group_off holds, no read leaves `hits` / `seg_off` and no write leaves `out`.
#include "cid_kernels.hpp"

namespace cid {

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kInFlight = 16;   // counter rows a wave loads before it compares them: a long group is bound by load latency, not bandwidth

struct Best {
    uint32_t seg, hit, len, n_perfect;
    __device__ __forceinline__ void clear() { seg = kNone; hit = 0; len = 0; n_perfect = 0; }
    // a later candidate: it wins only with a strictly greater share
    __device__ __forceinline__ void offer(uint32_t s, uint32_t h, uint32_t l) {
        if (h == 0 || l == 0) return;
        if (seg == kNone || (uint64_t)h * len > (uint64_t)hit * l) { seg = s; hit = h; len = l; }
    }
    __device__ __forceinline__ void merge_later(const uint4 &o) {
        n_perfect += o.w;
        if (o.x != kNone) offer(o.x, o.y, o.z);
    }
};
}  // namespace

__global__ __launch_bounds__(kBlock) void k_nearest_groups(NearestParams q) {
    __shared__ uint4 part[kBlock / kWave][kNearestGroups][kWave];
    __shared__ uint64_t s_go[kNearestGroups + 1];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.y * kWave + lane;
    const bool live = c < q.n_colors;
    const uint64_t g0 = (uint64_t)blockIdx.x * kNearestGroups;            // first group of the block, relative to q.group_off
    const uint32_t n_gl = q.n_groups - g0 < kNearestGroups ? (uint32_t)(q.n_groups - g0) : (uint32_t)kNearestGroups;

    if (threadIdx.x <= kNearestGroups) {   // the block's group boundaries, clamped into the launch's segment range
        const uint64_t i = g0 + (threadIdx.x < n_gl ? threadIdx.x : n_gl);
        uint64_t v = q.group_off[i];
        v = v < q.s_lo ? q.s_lo : v;
        s_go[threadIdx.x] = v > q.s_hi ? q.s_hi : v;
    }
#pragma unroll
    for (int g = 0; g < kNearestGroups; ++g) part[wave][g][lane] = make_uint4(kNone, 0u, 0u, 0u);
    __syncthreads();

    const uint64_t a = s_go[0], b = s_go[n_gl];
    const uint64_t n = b > a ? b - a : 0;
    const uint64_t per = (n + kBlock / kWave - 1) / (kBlock / kWave);
    const uint64_t w0 = a + (uint64_t)wave * per < b ? a + (uint64_t)wave * per : b;
    const uint64_t w1 = w0 + per < b ? w0 + per : b;

    Best best;
    best.clear();
    uint32_t gl = 0;   // wave-uniform: the local group whose running best sits in `best`
    const uint32_t *col = q.hits + (live ? c : 0u);
    auto length = [&](uint64_t s) { return (uint32_t)(q.seg_off[s - q.s_lo + 1] - q.seg_off[s - q.s_lo]); };
    auto take = [&](uint64_t s, uint32_t h, uint32_t len) {
        // the group of segment s: the last of the block's groups that starts at or before s (empty groups are stepped over)
        if (gl + 1 < n_gl && s >= s_go[gl + 1]) {
            part[wave][gl][lane] = make_uint4(best.seg, best.hit, best.len, best.n_perfect);
            best.clear();
            do ++gl; while (gl + 1 < n_gl && s >= s_go[gl + 1]);
        }
        best.offer((uint32_t)s, h, len);
        if (len && h == len) ++best.n_perfect;
    };
    uint64_t s = w0;
    for (; s + kInFlight <= w1; s += kInFlight) {   // kInFlight rows in flight
        // every load of the batch is issued before the first compare: no branch and no dependent address between them (a lane past the
        // last colour reads column 0 and counts nothing; the lengths come from one run of kInFlight + 1 offsets)
        uint32_t h[kInFlight];
        uint64_t o[kInFlight + 1];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) h[j] = col[(s + j - q.s_lo) * q.n_colors];
#pragma unroll
        for (int j = 0; j <= kInFlight; ++j) o[j] = q.seg_off[s - q.s_lo + j];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) take(s + j, live ? h[j] : 0u, (uint32_t)(o[j + 1] - o[j]));
    }
    for (; s < w1; ++s) take(s, live ? col[(s - q.s_lo) * q.n_colors] : 0u, length(s));
    part[wave][gl][lane] = make_uint4(best.seg, best.hit, best.len, best.n_perfect);
    __syncthreads();

    // wave g: the cell of local group g (the earlier launches' winner, or the preset) and the four partials, earliest first
    if ((uint32_t)wave < n_gl && live) {
        uint4 *cell = q.out + (q.g_base + g0 + wave) * q.n_colors + c;
        const uint4 old = *cell;
        Best r{old.x, old.y, old.z, old.w};
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) r.merge_later(part[w][wave][lane]);
        *cell = make_uint4(r.seg, r.hit, r.len, r.n_perfect);
    }
}

// every cell {CID_NEAREST_NONE, 0, 0, 0}
__global__ __launch_bounds__(256) void k_nearest_preset(uint4 *out, uint64_t n_cells) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_cells) out[i] = make_uint4(kNone, 0u, 0u, 0u);
}

hipError_t launch_nearest_groups(const NearestParams &q, hipStream_t stream) {
    if (q.n_groups == 0 || q.n_colors == 0) return hipSuccess;
    const uint64_t gx = (q.n_groups + kNearestGroups - 1) / kNearestGroups;
    if (gx >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nearest_groups, dim3((unsigned)gx, (q.n_colors + kWave - 1) / kWave), dim3(kBlock), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_nearest_preset(void *out, uint64_t n_cells, hipStream_t stream) {
    if (n_cells == 0) return hipSuccess;
    if ((n_cells + 255) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nearest_preset, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, (uint4 *)out, n_cells);
    return hipGetLastError();
}

}  // namespace cid
