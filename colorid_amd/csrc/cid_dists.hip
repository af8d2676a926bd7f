// `colorid dists` kernels for MI355X (gfx950): the pairwise allele distances of a cgMLST table (cid_dists_*).  The table is n_acc x n_loci
// u32 allele codes, 0 = no call.  For two accessions i, j:  compared = #loci both called,  differ = #loci both called with unequal codes.
// The device keeps the codes TRANSPOSED, T[locus][accession] with the accession stride padded to a multiple of 64 (the padding is zero =
// missing), and per accession the bitmask of its called loci, maskT[word][accession].  Integer counts only: exact, whatever the schedule.
#include "cid_kernels.hpp"

namespace cid {

constexpr uint32_t kDistsTile = 64;     // accessions per side of a workgroup's tile of pairs
constexpr uint32_t kDistsChunk = 32;    // loci staged in LDS at a time: 2 x 32 x 64 x 4 = 16 KiB
constexpr uint32_t kMissRow = 0xFFFFFFFFu, kMissCol = 0xFFFFFFFEu;   // what a missing cell is staged as on either side of a tile
static_assert(kBlock == 256 && kWave == 64, "k_dists_*: 256 threads = 16 x 16 blocks of 4 x 4 pairs, staged by four waves");

// One upload piece — the accessions [a0, a0 + na) as the caller holds them, row-major na x L — into T, 64 x 64 tiles through LDS so that
// both the reads (along the loci) and the writes (along the accessions) are contiguous.  A code of 0xFFFFFFFE / 0xFFFFFFFF sets *err.
// Grid: (ceil(L / 64), ceil(na / 64)).
__global__ __launch_bounds__(kBlock) void k_dists_put(const uint32_t *codes, uint32_t a0, uint32_t na, uint32_t L, uint32_t *T, uint64_t Ap,
                                                      uint32_t *err) {
    __shared__ uint32_t tile[kDistsTile][kDistsTile + 1];
    const uint32_t x = threadIdx.x & 63u, y = threadIdx.x >> 6;
    const uint32_t l_base = blockIdx.x * kDistsTile, a_base = blockIdx.y * kDistsTile;
    bool bad = false;
    for (uint32_t r = y; r < kDistsTile; r += 4) {
        const uint32_t a = a_base + r, l = l_base + x;
        const uint32_t v = (a < na && l < L) ? codes[(uint64_t)a * L + l] : 0u;
        bad |= v >= kMissCol;
        tile[r][x] = v;
    }
    if (bad) atomicOr(err, 1u);
    __syncthreads();
    for (uint32_t r = y; r < kDistsTile; r += 4) {
        const uint32_t l = l_base + r, a = a_base + x;
        if (l < L && a < na) T[(uint64_t)l * Ap + a0 + a] = tile[x][r];
    }
}

// The called-loci bitmasks of the same piece: one wave per (accession, 64 loci), bit b of word w = locus 64 w + b is called.
__global__ __launch_bounds__(kBlock) void k_dists_mask(const uint32_t *codes, uint32_t a0, uint32_t na, uint32_t L, uint32_t W,
                                                       unsigned long long *maskT, uint64_t Ap) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t g = (uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (g >= (uint64_t)na * W) return;   // wave-uniform
    const uint32_t a = (uint32_t)(g / W), w = (uint32_t)(g % W);
    const uint32_t l = w * 64u + lane;
    const uint32_t v = l < L ? codes[(uint64_t)a * L + l] : 0u;
    const unsigned long long m = __ballot(v != 0u);
    if (lane == 0) maskT[(uint64_t)w * Ap + a0 + a] = m;
}

// A workgroup owns the 64 x 64 pairs (row accessions row0 + 64 by .. + 63) x (column accessions 64 bx .. + 63) and walks the loci in
// chunks of 32 staged in LDS as [locus][64 accessions], one array per side; a missing cell is staged as kMissRow on the row side and
// kMissCol on the column side, two values no code may have (cid_dists_create refuses them), so it equals nothing — the diagonal tile
// included — and the inner loop is equal += (a == b) and nothing else.  Thread (ty, tx) of the 16 x 16 keeps the 4 x 4 pairs (4 ty .. + 3)
// x (4 tx .. + 3) in registers and reads its four row codes and its four column codes of a locus with one 16-byte LDS read each: a wave's
// column addresses are 256 contiguous bytes, its row addresses four broadcasts — no bank conflict with the rows 256 bytes apart.
// The next chunk's cells are fetched into registers before the current one is counted.  Loci past L are staged as missing (chunk tail);
// row accessions past A are staged as missing and never stored, column accessions past A read T's zero padding (tile tails).
// compared[i][j] = popcount(mask_i & mask_j) over the W mask words, differ = compared - equal.
// BOUND: equal <= compared <= L < 2^32.
// The walk is one body (dists_tile_walk) with five epilogues: k_dists_tile stores the counts, k_dists_best keeps a row's best pair,
// k_dists_within appends the pairs under a threshold to a list, k_dists_closest keeps a row's k best pairs of the tile, k_dists_hist
// counts the pairs by compared and by differ.
__device__ __forceinline__ void dists_tile_walk(const DistsParams &p, uint32_t ty, uint32_t tx, uint64_t row_base, uint64_t col_base,
                                                uint32_t (&eq)[4][4], uint32_t (&cmp)[4][4]) {
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kDistsChunk][kDistsTile];
    __shared__ __attribute__((aligned(16))) uint32_t s_col[kDistsChunk][kDistsTile];
    const uint32_t t = threadIdx.x;
    const uint32_t sx = t & 63u, sl = t >> 6;   // staging: wave sl takes the loci sl, sl + 4, .. of a chunk, lane sx the accession
    const bool row_ok = row_base + sx < p.A;
    constexpr uint32_t kPer = kDistsChunk / 4;
    uint32_t fr[kPer], fc[kPer];
    auto fetch = [&](uint32_t l0) {
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            const uint32_t l = l0 + sl + 4u * i;
            fr[i] = (l < p.L && row_ok) ? p.T[(uint64_t)l * p.Ap + row_base + sx] : 0u;
            fc[i] = l < p.L ? p.T[(uint64_t)l * p.Ap + col_base + sx] : 0u;
        }
    };
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) eq[r][c] = 0;
    fetch(0);
    for (uint32_t l0 = 0; l0 < p.L; l0 += kDistsChunk) {
        __syncthreads();   // the chunk before has been counted by every wave
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
            s_row[sl + 4u * i][sx] = fr[i] ? fr[i] : kMissRow;
            s_col[sl + 4u * i][sx] = fc[i] ? fc[i] : kMissCol;
        }
        __syncthreads();
        if (p.L - l0 > kDistsChunk) fetch(l0 + kDistsChunk);
#pragma unroll 2
        for (uint32_t l = 0; l < kDistsChunk; ++l) {
            const uint4 a4 = *reinterpret_cast<const uint4 *>(&s_row[l][4u * ty]);
            const uint4 b4 = *reinterpret_cast<const uint4 *>(&s_col[l][4u * tx]);
            const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) eq[r][c] += a[r] == b[c] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) cmp[r][c] = 0;
    for (uint32_t w = 0; w < p.W; ++w) {
        const unsigned long long *m = p.maskT + (uint64_t)w * p.Ap;
        unsigned long long mi[4], mj[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t i = row_base + 4u * ty + (uint32_t)r;
            mi[r] = i < p.A ? m[i] : 0ull;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) mj[c] = m[col_base + 4u * tx + (uint32_t)c];   // (< Ap: the padding's masks are zero)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) cmp[r][c] += (uint32_t)__popcll(mi[r] & mj[c]);
    }
}

__global__ __launch_bounds__(kBlock) void k_dists_tile(DistsParams p) {
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t col_base = (uint64_t)blockIdx.x * kDistsTile, row_base = (uint64_t)p.row0 + (uint64_t)blockIdx.y * kDistsTile;
    uint32_t eq[4][4], cmp[4][4];
    dists_tile_walk(p, ty, tx, row_base, col_base, eq, cmp);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t local = (uint64_t)blockIdx.y * kDistsTile + 4u * ty + (uint32_t)r;   // the row within [row0, row0 + n_rows)
        if (local >= p.n_rows) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = col_base + 4u * tx + (uint32_t)c;
            if (j >= p.A) continue;
            p.differ[local * p.A + j] = cmp[r][c] - eq[r][c];
            if (p.compared) p.compared[local * p.A + j] = cmp[r][c];
        }
    }
}

// One Borůvka round (cid_dists_best): the same walk, and instead of the store every row accession i keeps the best pair {i, j} over the
// columns j of another component (b.comp[j] != b.comp[i], which also excludes j == i) that share at least b.min_compared loci with it.
// Best = least (differ, L - compared, j): fewest differences, then most shared loci, then the lower accession — for a fixed i that is the
// order of the edge key (differ, -compared, min(i, j), max(i, j)).  The three fields are packed into one u64,
//     key = differ << (bits_l + bits_a) | (L - compared) << bits_a | j,     bits_l = bits of L, bits_a = bits of A - 1
// (launch_dists_best refuses a shape whose 2 bits_l + bits_a exceed 64), so the least key is the best pair and a row's result is one
// 64-bit minimum: over a thread's 4 columns in registers, over the row's 16 tx lanes — adjacent lanes of one wave — by four xor
// shuffles, and over the A / 64 column tiles by one atomicMin of lane tx = 0 on b.best[i], which the caller has set to kDistsNoBest.
// No pair gives that value: a candidate has compared >= 1, so its middle field is below L and its key below 2^64 - 1.  The atomic is
// skipped when the word already holds less; it only ever decreases, so a stale read costs an atomic and never a result.
// Tails: a row past A is never reported; a column past A has zero masks, compared = 0 < min_compared (>= 1), and is no candidate.
__global__ __launch_bounds__(kBlock) void k_dists_best(DistsParams p, DistsBestParams b) {
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t col_base = (uint64_t)blockIdx.x * kDistsTile, row_base = (uint64_t)p.row0 + (uint64_t)blockIdx.y * kDistsTile;
    uint32_t eq[4][4], cmp[4][4];
    dists_tile_walk(p, ty, tx, row_base, col_base, eq, cmp);
    uint32_t cj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint64_t j = col_base + 4u * tx + (uint32_t)c;
        cj[c] = j < p.A ? b.comp[j] : 0u;   // (past A: compared = 0 keeps it out whatever the label)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t i = row_base + 4u * ty + (uint32_t)r;   // uniform over the 16 tx lanes of the row
        const uint32_t ci = i < p.A ? b.comp[i] : 0u;
        unsigned long long key = kDistsNoBest;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = col_base + 4u * tx + (uint32_t)c;
            const unsigned long long k = ((unsigned long long)(cmp[r][c] - eq[r][c]) << b.shift_differ) |
                                         ((unsigned long long)(p.L - cmp[r][c]) << b.shift_compared) | j;
            if (cmp[r][c] >= b.min_compared && cj[c] != ci && k < key) key = k;
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const unsigned long long o = __shfl_xor(key, m, 16);
            key = o < key ? o : key;
        }
        if (tx == 0 && i < p.A && key < b.best[i]) atomicMin(&b.best[i], key);
    }
}

// The neighbour list (cid_dists_within): the same walk, and instead of the store a pair (i, j) is a HIT when i is a row of the launch,
// j < A, j != i, compared >= w.min_compared (>= 1), differ <= w.max_differ and — w.upper — j > i; every hit goes out as one 16-byte
// entry {i, j, differ, compared}, compacted.  Slots: a thread counts its hits (a 16-bit mask of its 4 x 4), a wave scans the counts with
// six shuffles, the four wave totals go through LDS, and thread 0 takes the workgroup's range with ONE 64-bit atomicAdd on *w.cursor —
// none when the workgroup has no hit.  An entry whose slot is at or past w.cap is not stored and the cursor keeps counting: after the
// launch it holds the exact number of hits whatever the capacity (cap = 0: a count, w.list is not touched).  Which slot a hit gets
// depends on the order of the atomics; the set of entries does not, and the caller sorts.
// Upper mode: a workgroup whose tile lies wholly on or below the diagonal — its last column col_base + 63 <= its first row, the real
// one: row0 need not be a multiple of 64 — returns before the walk; the test is uniform over the workgroup and precedes every barrier.
// Tails: a row past n_rows (so past A) is never reported; a column past A has zero masks, compared = 0 < min_compared, and is no hit.
__global__ __launch_bounds__(kBlock) void k_dists_within(DistsParams p, DistsWithinParams w) {
    __shared__ uint32_t s_wave[kBlock / kWave];
    __shared__ unsigned long long s_base;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t col_base = (uint64_t)blockIdx.x * kDistsTile, row_base = (uint64_t)p.row0 + (uint64_t)blockIdx.y * kDistsTile;
    if (w.upper && col_base + (kDistsTile - 1) <= row_base) return;
    uint32_t eq[4][4], cmp[4][4];
    dists_tile_walk(p, ty, tx, row_base, col_base, eq, cmp);
    uint32_t hits = 0;   // bit 4 r + c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t local = (uint64_t)blockIdx.y * kDistsTile + 4u * ty + (uint32_t)r;   // the row within [row0, row0 + n_rows)
        const uint64_t i = row_base + 4u * ty + (uint32_t)r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = col_base + 4u * tx + (uint32_t)c;
            const bool hit = local < p.n_rows && j < p.A && j != i && cmp[r][c] >= w.min_compared && cmp[r][c] - eq[r][c] <= w.max_differ &&
                             (!w.upper || j > i);
            hits |= hit ? 1u << (4 * r + c) : 0u;
        }
    }
    const uint32_t mine = (uint32_t)__popc(hits), lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < (int)kWave; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, kWave);
        if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t v = 0; v < kBlock / kWave; ++v) {
        before += v < wave ? s_wave[v] : 0u;
        total += s_wave[v];
    }
    if (total == 0) return;   // uniform over the workgroup
    if (threadIdx.x == 0) s_base = atomicAdd(w.cursor, (unsigned long long)total);
    __syncthreads();
    unsigned long long slot = s_base + before + (inc - mine);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!(hits >> (4 * r + c) & 1u)) continue;
            if (slot < w.cap)
                w.list[slot] = make_uint4((uint32_t)(row_base + 4u * ty + (uint32_t)r), (uint32_t)(col_base + 4u * tx + (uint32_t)c),
                                          cmp[r][c] - eq[r][c], cmp[r][c]);
            ++slot;
        }
}

// The K nearest (cid_dists_closest): the same walk, and instead of the store every pair of the tile becomes the key of k_dists_best —
// differ << shift_differ | (L - compared) << shift_compared | j, the same shifts — or kDistsNoBest when it is no CANDIDATE: a row past
// the launch, j >= A, j == i, compared < q.min_compared (>= 1) or differ > q.max_differ.  For a fixed row the keys of its candidates are
// distinct (j is part of them) and their order is the order asked for: differ ascending, compared descending, j ascending.  A row's 64
// columns of the tile sit in 16 adjacent tx lanes x 4 registers, and the tile's q.k (<= 64) least keys of the row come out in q.k rounds
// of "the least key at or above floor": a minimum over the thread's four registers, four xor shuffles over the row's 16 lanes, and
// floor = that minimum + 1 — the order is strict, so nothing is removed between rounds; once the minimum is kDistsNoBest the floor stays
// there and so does every later round's result.  The four rows of a thread go through a round together (16 keys, 32 registers: the
// walk's counters are dead by then).  Lane tx = 0 stores round n of local row r to part[(r * tiles + bx) * k + n]: every slot of every
// row of the launch is written by exactly one lane — part needs no preset, there is no atomic and no result depends on scheduling.
// k_dists_closest_merge puts a row's tiles together.
__global__ __launch_bounds__(kBlock) void k_dists_closest(DistsParams p, DistsClosestParams q) {
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint64_t col_base = (uint64_t)blockIdx.x * kDistsTile, row_base = (uint64_t)p.row0 + (uint64_t)blockIdx.y * kDistsTile;
    uint32_t eq[4][4], cmp[4][4];
    dists_tile_walk(p, ty, tx, row_base, col_base, eq, cmp);
    unsigned long long key[4][4], floor[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t local = (uint64_t)blockIdx.y * kDistsTile + 4u * ty + (uint32_t)r;   // the row within [row0, row0 + n_rows)
        const uint64_t i = row_base + 4u * ty + (uint32_t)r;
        floor[r] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t j = col_base + 4u * tx + (uint32_t)c;
            const uint32_t differ = cmp[r][c] - eq[r][c];
            const bool cand = local < p.n_rows && j < p.A && j != i && cmp[r][c] >= q.min_compared && differ <= q.max_differ;
            key[r][c] = cand ? ((unsigned long long)differ << q.shift_differ) | ((unsigned long long)(p.L - cmp[r][c]) << q.shift_compared) | j
                             : kDistsNoBest;
        }
    }
    const uint64_t tiles = gridDim.x;
    for (uint32_t n = 0; n < q.k; ++n) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned long long m = kDistsNoBest;
#pragma unroll
            for (int c = 0; c < 4; ++c) m = (key[r][c] >= floor[r] && key[r][c] < m) ? key[r][c] : m;
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) {
                const unsigned long long o = __shfl_xor(m, x, 16);
                m = o < m ? o : m;
            }
            floor[r] = m == kDistsNoBest ? m : m + 1;
            const uint64_t local = (uint64_t)blockIdx.y * kDistsTile + 4u * ty + (uint32_t)r;
            if (tx == 0 && local < p.n_rows) q.part[(local * tiles + blockIdx.x) * q.k + n] = m;
        }
    }
}

// One level of the merge: `in` holds, per row, n_lists lists of k keys, each ascending with kDistsNoBest behind its last key, and no key
// but that one twice in a row; a wave takes 64 adjacent lists of a row — lane t the list 64 g + t, its head in a register — and gives
// their k least keys, ascending, as list g of the row in `out` (n_groups = ceil(n_lists / 64) lists a row).  A round is the minimum of
// the 64 heads by six xor shuffles; the one lane whose head it is moves on to its list's next key (none when it is kDistsNoBest: every
// head is, and stays).  Lane n keeps round n's key and the k of them go out in one store.  Level by level a row's lists become one: its
// k nearest.  Nothing is shared between waves: no LDS, no barrier, no atomic.
__global__ __launch_bounds__(kBlock) void k_dists_closest_merge(const unsigned long long *in, unsigned long long *out, uint64_t n_rows,
                                                                uint64_t n_lists, uint64_t n_groups, uint32_t k) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t job = (uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (job >= n_rows * n_groups) return;   // wave-uniform
    const uint64_t row = job / n_groups, g = job % n_groups;
    const uint64_t t = g * kWave + lane;
    const unsigned long long *list = in + (row * n_lists + (t < n_lists ? t : 0)) * k;
    uint32_t cur = 0;
    unsigned long long head = t < n_lists ? list[0] : kDistsNoBest, mine = kDistsNoBest;
    for (uint32_t n = 0; n < k; ++n) {
        unsigned long long m = head;
#pragma unroll
        for (int x = 1; x < (int)kWave; x <<= 1) {
            const unsigned long long o = __shfl_xor(m, x, kWave);
            m = o < m ? o : m;
        }
        if (lane == n) mine = m;
        if (head == m && m != kDistsNoBest) {
            ++cur;
            head = cur < k ? list[cur] : kDistsNoBest;
        }
    }
    if (lane < k) out[job * k + lane] = mine;
}

// The histograms (cid_dists_hist): the same walk, and instead of the store a pair (i, j) is COUNTED when i is a row of the launch, j < A,
// j != i and — h.upper — j > i: it adds 1 to compared_hist[compared] whatever h.min_compared is (bin 0: the pairs without a common locus)
// and, when compared >= h.min_compared (>= 1), 1 to differ_hist[differ].  Bins 0 .. L.  A column past A is dropped by j < A and by nothing
// else: its zero masks give compared = 0, which is a bin.
// Where the counts go: a workgroup keeps the bins 0 .. kDistsHistWindow - 1 of both histograms as u32 in LDS (2 x 16 KiB beside the walk's
// 16 KiB) with one LDS atomic per count — 2 x 4 096 a tile against the walk's 2 L LDS reads and 16 L compares a thread — and walks SEVERAL
// tiles, a contiguous share of the launch's tile list, before it adds its non-zero bins to the global u64 histograms, one 64-bit atomic
// a bin, once.  A count for a bin at or past the window (L >= 4 096) goes to the global word at once: the one path there is, slow and exact.
// The tile list: tile t of full mode is (row tile t / C, column tile t % C), C = Ap / 64.  Upper mode lists only the tiles not wholly on
// or below the diagonal: those of k_dists_within's test with the real first row — column tile bx of row tile by stays when 64 bx + 63 >
// row0 + 64 by, that is bx >= q0 + by with q0 = (row0 + 1) / 64 — so row tile by has n0 - by of them, n0 = C - q0 (none at all for a last
// row tile that begins at A - 1 = 64 C - 1), and before it lie by n0 - by (by - 1) / 2: a workgroup finds its first tile by bisection
// and steps from there.  Workgroup g of G takes the tiles [g share + min(g, rest), ..) — share = n_tiles / G, rest = n_tiles % G, one
// more for g < rest; everything about the list is uniform over the workgroup.
// BOUND: a tile adds at most 64 x 64 to one bin, a workgroup owns at most kDistsHistMaxShare = (2^32 - 1) / 4 096 tiles
// (launch_dists_hist grows the grid beyond that), so no u32 bin wraps; the u64 bins hold at most A^2 < 2^64.
static_assert(kDistsHistMaxShare * kDistsTile * kDistsTile <= 0xFFFFFFFFull, "k_dists_hist: a workgroup's u32 bins");
__device__ __forceinline__ uint64_t dists_hist_before(uint64_t by, uint64_t n0) { return by * n0 - by * (by - 1) / 2; }

__global__ __launch_bounds__(kBlock) void k_dists_hist(DistsParams p, DistsHistParams h) {
    __shared__ uint32_t s_differ[kDistsHistWindow], s_compared[kDistsHistWindow];
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    for (uint32_t b = threadIdx.x; b < kDistsHistWindow; b += kBlock) s_differ[b] = s_compared[b] = 0u;
    __syncthreads();
    const uint64_t C = p.Ap / kDistsTile, R = ((uint64_t)p.n_rows + kDistsTile - 1) / kDistsTile;
    const uint64_t q0 = ((uint64_t)p.row0 + 1u) / kDistsTile, n0 = C - q0;
    const uint64_t share = h.n_tiles / gridDim.x, rest = h.n_tiles % gridDim.x, g = blockIdx.x;
    const uint64_t t0 = g * share + (g < rest ? g : rest), n_mine = share + (g < rest ? 1u : 0u);
    uint64_t by, bx;
    if (h.upper) {
        uint64_t lo = 0, hi = R - 1;   // the last row tile that begins at or before t0
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) / 2;
            if (dists_hist_before(mid, n0) <= t0) lo = mid;
            else hi = mid - 1;
        }
        by = lo;
        bx = q0 + by + (t0 - dists_hist_before(by, n0));
    } else {
        by = t0 / C;
        bx = t0 % C;
    }
    for (uint64_t n = 0; n < n_mine; ++n) {
        const uint64_t col_base = bx * kDistsTile, row_base = (uint64_t)p.row0 + by * kDistsTile;
        uint32_t eq[4][4], cmp[4][4];
        dists_tile_walk(p, ty, tx, row_base, col_base, eq, cmp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint64_t local = by * kDistsTile + 4u * ty + (uint32_t)r;   // the row within [row0, row0 + n_rows)
            const uint64_t i = row_base + 4u * ty + (uint32_t)r;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint64_t j = col_base + 4u * tx + (uint32_t)c;
                if (!(local < p.n_rows && j < p.A && j != i && (!h.upper || j > i))) continue;
                const uint32_t compared = cmp[r][c], differ = cmp[r][c] - eq[r][c];
                if (compared < kDistsHistWindow) atomicAdd(&s_compared[compared], 1u);
                else atomicAdd(&h.compared_hist[compared], 1ull);
                if (compared < h.min_compared) continue;
                if (differ < kDistsHistWindow) atomicAdd(&s_differ[differ], 1u);
                else atomicAdd(&h.differ_hist[differ], 1ull);
            }
        }
        if (++bx == C) {
            ++by;
            bx = h.upper ? q0 + by : 0;
        }
    }
    __syncthreads();
    const uint32_t in_lds = p.L < kDistsHistWindow ? p.L + 1u : kDistsHistWindow;   // the bins there are, of those kept here
    for (uint32_t b = threadIdx.x; b < in_lds; b += kBlock) {
        const uint32_t nd = s_differ[b], nc = s_compared[b];
        if (nd) atomicAdd(&h.differ_hist[b], (unsigned long long)nd);
        if (nc) atomicAdd(&h.compared_hist[b], (unsigned long long)nc);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

hipError_t launch_dists_put(const uint32_t *d_codes, uint32_t a0, uint32_t na, uint32_t L, uint32_t *T, unsigned long long *maskT, uint64_t Ap,
                            uint32_t *d_err, hipStream_t stream) {
    if (na == 0 || L == 0) return hipSuccess;
    if ((na + kDistsTile - 1) / kDistsTile > kDistsMaxRowTiles) return hipErrorInvalidValue;
    const uint32_t W = (L + 63u) / 64u;
    hipLaunchKernelGGL(k_dists_put, dim3((L + kDistsTile - 1) / kDistsTile, (na + kDistsTile - 1) / kDistsTile), dim3(kBlock), 0, stream, d_codes, a0,
                       na, L, T, Ap, d_err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t waves = (uint64_t)na * W;
    hipLaunchKernelGGL(k_dists_mask, dim3((unsigned)((waves + 3) / 4)), dim3(kBlock), 0, stream, d_codes, a0, na, L, W, maskT, Ap);
    return hipGetLastError();
}

hipError_t launch_dists_tile(const DistsParams &p, hipStream_t stream) {
    if (p.n_rows == 0 || p.A == 0) return hipSuccess;
    const uint32_t row_tiles = (p.n_rows + kDistsTile - 1) / kDistsTile;
    if (row_tiles > kDistsMaxRowTiles || (uint64_t)p.row0 + p.n_rows > p.A) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dists_tile, dim3((unsigned)(p.Ap / kDistsTile), row_tiles), dim3(kBlock), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_dists_within(const DistsParams &p, const DistsWithinParams &w, hipStream_t stream) {
    if (p.n_rows == 0 || p.A == 0) return hipSuccess;
    const uint32_t row_tiles = (p.n_rows + kDistsTile - 1) / kDistsTile;
    if (row_tiles > kDistsMaxRowTiles || (uint64_t)p.row0 + p.n_rows > p.A) return hipErrorInvalidValue;
    if (w.min_compared == 0 || !w.cursor || (!w.list && w.cap)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dists_within, dim3((unsigned)(p.Ap / kDistsTile), row_tiles), dim3(kBlock), 0, stream, p, w);
    return hipGetLastError();
}

bool dists_best_shifts(uint32_t A, uint32_t L, uint32_t *shift_differ, uint32_t *shift_compared) {
    uint32_t bits_l = 0, bits_a = 0;
    while (bits_l < 32 && (L >> bits_l)) ++bits_l;                       // ceil(log2(L + 1))
    while (bits_a < 32 && A && ((A - 1) >> bits_a)) ++bits_a;            // ceil(log2 A)
    *shift_compared = bits_a;
    *shift_differ = bits_a + bits_l;
    return 2 * bits_l + bits_a <= 64;
}

hipError_t launch_dists_best(DistsParams p, DistsBestParams b, hipStream_t stream) {
    if (p.A == 0 || p.L == 0) return hipSuccess;
    if (!dists_best_shifts(p.A, p.L, &b.shift_differ, &b.shift_compared) || b.min_compared == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(b.best, 0xFF, 8ull * p.A, stream);
    p.differ = p.compared = nullptr;
    const uint64_t per = 64ull * kDistsMaxRowTiles;   // rows a launch
    for (uint64_t r0 = 0; r0 < p.A && e == hipSuccess; r0 += per) {
        p.row0 = (uint32_t)r0;
        p.n_rows = (uint32_t)std::min<uint64_t>(per, p.A - r0);
        hipLaunchKernelGGL(k_dists_best, dim3((unsigned)(p.Ap / kDistsTile), (p.n_rows + kDistsTile - 1) / kDistsTile), dim3(kBlock), 0, stream, p, b);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_dists_closest(const DistsParams &p, DistsClosestParams q, hipStream_t stream) {
    if (p.n_rows == 0 || p.A == 0) return hipSuccess;
    const uint32_t row_tiles = (p.n_rows + kDistsTile - 1) / kDistsTile;
    if (row_tiles > kDistsMaxRowTiles || (uint64_t)p.row0 + p.n_rows > p.A) return hipErrorInvalidValue;
    if (q.k == 0 || q.k > kDistsClosestMax || q.min_compared == 0 || !q.part) return hipErrorInvalidValue;
    if (!dists_best_shifts(p.A, p.L, &q.shift_differ, &q.shift_compared)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dists_closest, dim3((unsigned)(p.Ap / kDistsTile), row_tiles), dim3(kBlock), 0, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_dists_closest_merge(const unsigned long long *in, unsigned long long *out, uint64_t n_rows, uint64_t n_lists, uint32_t k,
                                      hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    if (!in || !out || n_lists == 0 || k == 0 || k > kDistsClosestMax) return hipErrorInvalidValue;
    const uint64_t n_groups = (n_lists + kWave - 1) / kWave, blocks = (n_rows * n_groups + kBlock / kWave - 1) / (kBlock / kWave);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dists_closest_merge, dim3((unsigned)blocks), dim3(kBlock), 0, stream, in, out, n_rows, n_lists, n_groups, k);
    return hipGetLastError();
}

hipError_t launch_dists_hist(const DistsParams &p, DistsHistParams h, int n_cu, hipStream_t stream) {
    if (p.n_rows == 0 || p.A == 0 || p.L == 0) return hipSuccess;
    if ((uint64_t)p.row0 + p.n_rows > p.A || h.min_compared == 0 || !h.differ_hist || !h.compared_hist || n_cu <= 0) return hipErrorInvalidValue;
    const uint64_t C = p.Ap / kDistsTile, R = ((uint64_t)p.n_rows + kDistsTile - 1) / kDistsTile;
    const uint64_t n0 = C - ((uint64_t)p.row0 + 1u) / kDistsTile;   // upper: the tiles of the first row tile, one fewer each row tile down
    h.n_tiles = h.upper ? R * n0 - R * (R - 1) / 2 : R * C;
    if (h.n_tiles == 0) return hipSuccess;                          // (upper, and the one row is A - 1 = 64 C - 1)
    const uint64_t grid = std::max(std::min<uint64_t>(h.n_tiles, (uint64_t)n_cu * kDistsHistBlocksPerCu),
                                   (h.n_tiles + kDistsHistMaxShare - 1) / kDistsHistMaxShare);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dists_hist, dim3((unsigned)grid), dim3(kBlock), 0, stream, p, h);
    return hipGetLastError();
}

}  // namespace cid
