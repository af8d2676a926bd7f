// Index maintenance kernels for MI355X (gfx950): .bxi rows <-> dense matrix, Bloom insert (simple_bloom.rs:19-26).
#include <algorithm>

#include "cid_gather.hpp"
#include "cid_records.hpp"

namespace cid {

// ------------------------------------------------------------------------------------------------
// index maintenance

// .bxi rows -> dense matrix (src/bigsi.rs:59-63 feeds this): one thread per (row, u32 word)
__global__ void k_put_rows(uint32_t *mat32, uint32_t rs, const uint64_t *row_ids, const uint32_t *words, uint32_t w32,
                           uint64_t n_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * w32) return;
    const uint64_t r = i / w32, w = i % w32;
    mat32[row_ids[r] * (2ull * rs) + w] = words[i];
}

// The same from the file's own bytes, record by record (layout and check: cid_records.hpp).  The index takes the record's
// words [w_off, w_off + w32_take) — all of them, or its colour stripe of a wider file (cid_group_stripes_put_records).  One
// thread per (record, taken word); word 0's thread also checks the record against the FILE's shape (w32_rec words, n_colors
// bits): err[0] |= check_record's bits.
__global__ void k_put_records(uint32_t *mat32, uint32_t rs, const uint32_t *rec32, uint32_t w32_rec, uint32_t w_off, uint32_t w32_take,
                              uint64_t n_records, uint64_t bloom_size, uint32_t n_colors, uint32_t tail_mask, uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_records * w32_take) return;
    const uint64_t r = i / w32_take;
    const uint32_t w = (uint32_t)(i % w32_take);
    const uint32_t *rec = rec32 + r * record_words(w32_rec);
    const uint64_t row = record_row(rec);
    if (w == 0) {
        const uint32_t e = check_record(rec, row, w32_rec, n_colors, bloom_size, tail_mask);
        if (e) atomicOr(err, e);
    }
    if (row < bloom_size) mat32[row * (2ull * rs) + w] = rec[kRecordPayload + w_off + w];
}

// `merge`: the records of a file with n_colors_file colours OR-ed into a wider index through an increasing colour map.  The file
// colours that land in output word plan[j].w are one contiguous run [lo, lo + popc(mask)) — at most 32 bits over at most two source
// words: funnel-shifted together, then deposited into the bits of `mask` run by run (a software pdep).  One thread per (record, plan
// entry); entry 0's thread checks the record as k_put_records does.  A file holds each row once and the inputs go one after the other
// on one stream, so no two threads touch one word: a plain read-modify-write.
__global__ void k_put_records_mapped(uint32_t *mat32, uint32_t rs, const uint32_t *rec32, uint32_t w32_rec, const MergePlan *plan,
                                     uint32_t n_plan, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors_file, uint32_t tail_mask,
                                     uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_records * n_plan) return;
    const uint64_t r = i / n_plan;
    const uint32_t j = (uint32_t)(i % n_plan);
    const uint32_t *rec = rec32 + r * record_words(w32_rec);
    const uint64_t row = record_row(rec);
    if (j == 0) {
        const uint32_t e = check_record(rec, row, w32_rec, n_colors_file, bloom_size, tail_mask);
        if (e) atomicOr(err, e);
    }
    if (row >= bloom_size) return;
    const MergePlan p = plan[j];
    const uint32_t n = __builtin_popcount(p.mask);
    const uint32_t s0 = p.lo >> 5, sh = p.lo & 31u;
    const uint32_t lo_word = rec[kRecordPayload + s0];
    const uint32_t hi_word = sh + n > 32u ? rec[kRecordPayload + s0 + 1] : 0u;   // (the run ends inside the file's colours: s0 + 1 < w32_rec)
    uint32_t bits = __builtin_amdgcn_alignbit(hi_word, lo_word, sh);   // (hi:lo) >> sh
    bits &= low_bits(n);
    if (bits == 0) return;
    mat32[row * (2ull * rs) + p.w] |= deposit_bits(bits, p.mask);
}

// `subset`: the kept colours of a file with n_colors_file colours, packed into a narrower index — the inverse of the deposit above (a
// software pext).  One thread per (record, OUTPUT u32 word j): the word's 32 kept bits lie in a run of consecutive plan items (file
// words with a non-zero keep mask); the thread extracts each item's bits under its mask run by run, drops the `skip` bits of the first
// item that earlier output words took, and appends the rest where the word is filled so far — until 32 bits or the plan's end.  What
// overflows the word belongs to thread j + 1, which extracts it again.  Every output word of a put row is written once, by one thread,
// with a plain store: no atomics, no read-modify-write.  Only kept bits are ever appended, so the bits at and beyond the index's
// n_colors in the last word are zero.  Word 0's thread checks the record as k_put_records does, against the file's shape.
__global__ void k_put_records_subset(uint32_t *mat32, uint32_t rs, const uint32_t *rec32, uint32_t w32_rec, const SubsetWord *words,
                                     const SubsetItem *items, uint32_t w32_out, uint64_t n_records, uint64_t bloom_size,
                                     uint32_t n_colors_file, uint32_t tail_mask, uint32_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_records * w32_out) return;
    const uint64_t r = i / w32_out;
    const uint32_t j = (uint32_t)(i % w32_out);
    const uint32_t *rec = rec32 + r * record_words(w32_rec);
    const uint64_t row = record_row(rec);
    if (j == 0) {
        const uint32_t e = check_record(rec, row, w32_rec, n_colors_file, bloom_size, tail_mask);
        if (e) atomicOr(err, e);
    }
    if (row >= bloom_size) return;
    const SubsetWord p = words[j];
    uint32_t out = 0, filled = 0, drop = p.skip;
    for (uint32_t t = 0; t < p.n_items && filled < 32u; ++t) {
        const SubsetItem it = items[p.first + t];   // (it.s < w32_rec: the host made the items from the file's own words)
        uint32_t n;
        const uint32_t bits = extract_bits(rec[kRecordPayload + it.s], it.mask, n) >> drop;   // drop < n <= 32 for the first item, 0 afterwards
        out |= bits << filled;
        filled += n - drop;
        drop = 0;
    }
    mat32[row * (2ull * rs) + j] = out;
}

// `fold`: the records of a file whose Bloom size is a multiple of the index's, OR-ed into row (record's row) % bloom_size of the index —
// (h % m) % m' == h % m' when m' divides m, so this is the matrix `build` makes at the smaller size.  The piece was checked against the
// FILE's shape before this runs (k_pairs_check under stage_records: a refused piece leaves the matrix as it was), so nothing is checked
// here.  A workgroup takes recs_per_block consecutive records (at most 256): thread t reduces record t's row — the one 64-bit modulo of
// the record — into LDS; then the workgroup walks the tile's u32 words front to back, one coalesced load per payload word (the header
// and bit-count words share its lines and are stepped over), (record, word in record) advanced by the stride 256 without a division.
// Records r, r + m', r + 2m', ... of one piece land on one output row, in any order (a file written by the reference is in hash-map
// order): the OR is a no-return atomicOr on the matrix word; all-zero words are skipped.
constexpr uint32_t kFoldBlock = 256;
__global__ __launch_bounds__(kFoldBlock) void k_put_records_folded(uint32_t *mat32, uint32_t rs, const uint32_t *rec32, uint32_t w32_rec,
                                                                   uint32_t recs_per_block, uint64_t n_records, ModMagic mod) {
    __shared__ uint32_t dst_row[kFoldBlock];   // < bloom_size <= 2^32
    const uint64_t r0 = (uint64_t)blockIdx.x * recs_per_block;
    const uint32_t nr = n_records - r0 < recs_per_block ? (uint32_t)(n_records - r0) : recs_per_block;
    const uint32_t rw = (uint32_t)record_words(w32_rec);
    const uint32_t *tile = rec32 + r0 * rw;
    if (threadIdx.x < nr) dst_row[threadIdx.x] = (uint32_t)mod_m(record_row(tile + (uint64_t)threadIdx.x * rw), mod);
    __syncthreads();
    const uint32_t n_words = nr * rw;   // <= 256 * (6 + 32768)
    const uint32_t dq = kFoldBlock / rw, dr = kFoldBlock % rw;
    uint32_t r = threadIdx.x / rw, p = threadIdx.x % rw;
    for (uint32_t i = threadIdx.x; i < n_words; i += kFoldBlock) {
        if (p >= kRecordPayload && p < kRecordPayload + w32_rec) {
            const uint32_t v = tile[i];
            if (v) atomicOr(&mat32[(uint64_t)dst_row[r] * (2ull * rs) + (p - kRecordPayload)], v);
        }
        p += dr;
        r += dq;
        if (p >= rw) { p -= rw; ++r; }
    }
}

// `collapse`: the colours of a file with n_colors_file colours through an arbitrary many-to-one map into a narrower index: output bit
// (row, g) = OR of the record's bits over the members of g (the plan: cid_collapse.hpp), and in the same pass how many records have
// each file colour and each output colour set — every output row is complete once its record is applied.  The piece was checked against
// the FILE's shape before this runs (k_pairs_check under stage_records), so nothing is checked here.
// A workgroup of four waves walks tiles_per_block tiles of 64 consecutive records, lane = record.  p.staged (64 records fit in
// kGroupTileWords of LDS): the tile is loaded front to back, coalesced, and laid down at an odd stride of rws words per record, so that
// the 32 lanes of a half wave reading one word of 32 records hit 32 different banks; else (records of more than 121 words) a lane reads its
// record's words from global memory.  Wave v owns the file words and the output words == v mod 4: it evaluates its output words through the
// plan and stores each once, with a plain store — no atomics on the matrix; bits at and beyond n_colors stay zero because no item has
// them.  A column's count over the tile is __popcll(__ballot(bit)), 32 ballots a word, lane b keeping bit b's: staged, they add up in LDS
// counters that only the owning wave touches (plain read-modify-write) and are flushed once per workgroup, one 64-bit atomicAdd per
// non-zero column; unstaged, the counters do not fit and lanes 0..31 add the tile's counts to global memory (256 contiguous bytes).
// BOUND: an LDS counter takes at most 64 * tiles_per_block <= 2^22.
constexpr uint32_t kGroupBlock = 256, kGroupWaves = kGroupBlock / kWave;
constexpr uint32_t kGroupTileWords = 8192;   // 32 KiB of records; the counters beside them take at most 2 * 32 * 121 words
__device__ __forceinline__ uint32_t column_counts(uint32_t v, uint32_t lane) {   // lane b < 32 returns how many lanes have bit b of v set
    uint32_t mine = 0;
#pragma unroll 8   // (all 32 at once keep 32 ballots in scalar registers: they spill)
    for (uint32_t b = 0; b < 32u; ++b) {
        const uint32_t n = (uint32_t)__popcll(__ballot((v >> b) & 1u));
        if (lane == b) mine = n;
    }
    return mine;
}
__global__ __launch_bounds__(kGroupBlock) void k_put_records_grouped(GroupedParams p) {
    extern __shared__ __align__(16) uint32_t grouped_lds[];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const uint32_t rw = (uint32_t)record_words(p.w32_rec), rws = rw | 1u;
    uint32_t *tile = grouped_lds;                                      // [64][rws], staged only
    uint32_t *cnt = grouped_lds + (p.staged ? kWave * rws : 0u);      // [32 * w32_rec] file colours, [32 * w32_out] output colours, staged only
    const uint32_t n_cnt = p.staged && p.counts ? 32u * (p.w32_rec + p.w32_out) : 0u;
    for (uint32_t i = threadIdx.x; i < n_cnt; i += kGroupBlock) cnt[i] = 0;
    const uint64_t n_tiles = (p.n_records + kWave - 1) / kWave;
    const uint64_t tile0 = (uint64_t)blockIdx.x * p.tiles_per_block;
    const uint64_t tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
    for (uint64_t t = tile0; t < tile1; ++t) {
        const uint64_t r0 = t * kWave;
        const uint32_t nr = p.n_records - r0 < kWave ? (uint32_t)(p.n_records - r0) : kWave;
        const uint32_t *src = p.rec32 + r0 * rw;
        __syncthreads();   // the waves are done with the previous tile (and the counters are zero)
        if (p.staged) {
            const uint32_t n_words = nr * rw, dq = kGroupBlock / rw, dr = kGroupBlock % rw;
            uint32_t r = threadIdx.x / rw, q = threadIdx.x % rw;
            for (uint32_t i = threadIdx.x; i < n_words; i += kGroupBlock) {
                tile[r * rws + q] = src[i];
                q += dr;
                r += dq;
                if (q >= rw) { q -= rw; ++r; }
            }
        }
        __syncthreads();
        const bool have = lane < nr;
        const uint32_t *mine = src + (uint64_t)lane * rw;
        auto word = [&](uint32_t s) { return p.staged ? tile[lane * rws + kRecordPayload + s] : mine[kRecordPayload + s]; };
        if (p.counts)
            for (uint32_t s = wave; s < p.w32_rec; s += kGroupWaves) {
                const uint32_t n = column_counts(have ? word(s) : 0u, lane);
                if (lane < 32u) {
                    if (p.staged) cnt[32u * s + lane] += n;
                    else if (n && 32u * s + lane < p.n_colors_file) atomicAdd(&p.counts[32u * s + lane], (unsigned long long)n);
                }
            }
        const uint64_t row = have ? (p.staged ? (uint64_t)tile[lane * rws] | ((uint64_t)tile[lane * rws + 1] << 32) : record_row(mine)) : 0;
        for (uint32_t j = wave; j < p.w32_out; j += kGroupWaves) {
            uint32_t out = 0;
            if (have) {
                out = group_word(p.words[j], p.items, word);
                p.mat32[row * (2ull * p.rs) + j] = out;   // (row < bloom_size: the piece was checked)
            }
            if (!p.counts) continue;   // (the same in every lane)
            const uint32_t n = column_counts(out, lane);
            if (lane < 32u) {
                if (p.staged) cnt[32u * (p.w32_rec + j) + lane] += n;
                else if (n && 32u * j + lane < p.n_colors) atomicAdd(&p.counts[p.n_colors_file + 32u * j + lane], (unsigned long long)n);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_cnt; i += kGroupBlock) {
        const uint32_t n = cnt[i];
        if (n == 0) continue;
        const uint32_t f = 32u * p.w32_rec;
        if (i < f) { if (i < p.n_colors_file) atomicAdd(&p.counts[i], (unsigned long long)n); }
        else if (i - f < p.n_colors) atomicAdd(&p.counts[p.n_colors_file + (i - f)], (unsigned long long)n);
    }
}

// The same from a resident index of factor * m_dst rows and the same colours: one thread per (output row, u32 word) ORs the word of the
// source rows row, row + m_dst, row + 2 m_dst, ... in registers — neighbouring threads read neighbouring words of every source slice — and
// ORs the result into the output once; zero results (all-zero source rows) touch nothing.  With one chunk (gridDim.y == 1) each output
// word has one writer: a plain read-modify-write.  A small output with a large factor is split over gridDim.y chunks of the slices
// (chunk c takes slices c, c + gridDim.y, ...), whose threads share output words: atomicOr then.
__global__ void k_fold_rows(uint32_t *dst32, const uint32_t *src32, uint32_t rs, uint32_t w32, uint64_t m_dst, uint64_t factor) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m_dst * w32) return;
    const uint64_t row = i / w32;
    const uint32_t w = (uint32_t)(i % w32);
    uint32_t acc = 0;
    for (uint64_t s = blockIdx.y; s < factor; s += gridDim.y) acc |= src32[(s * m_dst + row) * (2ull * rs) + w];
    if (acc == 0) return;
    uint32_t *d = &dst32[row * (2ull * rs) + w];
    if (gridDim.y == 1) *d |= acc;
    else atomicOr(d, acc);
}

__global__ void k_get_rows(const uint32_t *mat32, uint32_t rs, const uint64_t *row_ids, uint32_t *words, uint32_t w32,
                           uint64_t n_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * w32) return;
    const uint64_t r = i / w32, w = i % w32;
    words[i] = mat32[row_ids[r] * (2ull * rs) + w];
}

// Bloom insert (src/simple_bloom.rs:19-26) straight into the transposed matrix (src/build.rs:116-128)
__global__ __launch_bounds__(kBlock) void k_insert_kmers(InsertParams p) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    uint32_t *img = reinterpret_cast<uint32_t *>(smem + (size_t)wave * kmer_img_bytes(p.k));
    const uint64_t n_tiles = (p.n_kmers + kWave - 1) / kWave;
    const uint64_t tile0 = (uint64_t)blockIdx.x * p.tiles_per_block;
    const uint64_t tile1 = tile0 + p.tiles_per_block < n_tiles ? tile0 + p.tiles_per_block : n_tiles;
    unsigned int *mat32 = reinterpret_cast<unsigned int *>(p.mat);
    for (uint64_t tile = tile0 + wave; tile < tile1; tile += kBlock / kWave) {
        const uint64_t first = tile * kWave;
        auto set_bit = [&](uint32_t c, uint64_t h) {
            const uint64_t row = mod_m(h, p.mod);
            atomicOr(&mat32[row * (2ull * p.rs) + (c >> 5)], 1u << (c & 31u));
        };
        if (p.codes) {
            if (first + lane < p.n_kmers) {
                const uint32_t c = p.colour_of_kmer ? p.colour_of_kmer[first + lane] : p.colour;
                uint64_t code = p.codes[first + lane];
                uint32_t klen = p.k;
                if (p.m_size) { code = minimizer_code(code, p.k, p.m_size); klen = p.m_size; }
                const uint64_t lsb = rev_fields(code, klen);
                if (c < p.n_colors) xxh3_seeds_from(CodeReader{lsb}, klen, p.n_hash, HashSel::of(p.mod), [&](uint32_t, uint64_t h) { set_bit(c, h); });
            }
            continue;
        }
        wave_lds_fence();
        stage_kmers(img, p.kmers, p.n_kmers, first, p.k, lane);
        wave_lds_fence();
        if (p.m_size) {  // ASCII k-mers into a minimizer index: byte-wise find_minimizer, then hash its m_size bytes
            uint32_t *mimg = reinterpret_cast<uint32_t *>(smem + (size_t)(kBlock / kWave) * kmer_img_bytes(p.k) + (size_t)wave * kmer_img_bytes(p.m_size));
            uint8_t *mimg8 = reinterpret_cast<uint8_t *>(mimg);
            const bool have = first + lane < p.n_kmers;
            if (have) {
                const uint8_t *seq = reinterpret_cast<const uint8_t *>(img) + (uint32_t)lane * p.k;
                const uint32_t cand = find_minimizer_bytes(seq, p.k, p.m_size);
                for (uint32_t t = 0; t < p.m_size; ++t) mimg8[(uint32_t)lane * p.m_size + t] = mini_byte(seq, cand, p.m_size, t);
            }
            wave_lds_fence();
            if (have) {
                const uint32_t c = p.colour_of_kmer ? p.colour_of_kmer[first + lane] : p.colour;
                if (c < p.n_colors)
                    xxh3_seeds(mimg, (uint32_t)lane * p.m_size, p.m_size, p.n_hash, HashSel::of(p.mod), [&](uint32_t, uint64_t h) { set_bit(c, h); });
            }
            continue;
        }
        if (first + lane < p.n_kmers) {
            const uint32_t c = p.colour_of_kmer ? p.colour_of_kmer[first + lane] : p.colour;
            if (c < p.n_colors) xxh3_seeds(img, (uint32_t)lane * p.k, p.k, p.n_hash, HashSel::of(p.mod), [&](uint32_t, uint64_t h) { set_bit(c, h); });
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

hipError_t launch_put_rows(uint64_t *mat, uint32_t rs, const uint64_t *d_row_ids, const uint32_t *d_words, uint32_t w32,
                           uint64_t n_rows, hipStream_t stream) {
    const uint64_t n = n_rows * w32;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_put_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<uint32_t *>(mat), rs, d_row_ids, d_words, w32, n_rows);
    return hipGetLastError();
}

hipError_t launch_put_records(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, uint32_t w_off, uint32_t w32_take,
                              uint64_t n_records, uint64_t bloom_size, uint32_t n_colors, uint32_t *d_err, hipStream_t stream) {
    const uint64_t n = n_records * w32_take;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_put_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(mat), rs, d_records,
                       w32_rec, w_off, w32_take, n_records, bloom_size, n_colors, tail_mask(n_colors), d_err);
    return hipGetLastError();
}

hipError_t launch_put_records_mapped(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, const MergePlan *d_plan,
                                     uint32_t n_plan, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors_file, uint32_t *d_err,
                                     hipStream_t stream) {
    const uint64_t n = n_records * n_plan;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_put_records_mapped, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(mat), rs,
                       d_records, w32_rec, d_plan, n_plan, n_records, bloom_size, n_colors_file, tail_mask(n_colors_file), d_err);
    return hipGetLastError();
}

hipError_t launch_put_records_subset(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, const SubsetWord *d_words,
                                     const SubsetItem *d_items, uint32_t w32_out, uint64_t n_records, uint64_t bloom_size,
                                     uint32_t n_colors_file, uint32_t *d_err, hipStream_t stream) {
    const uint64_t n = n_records * w32_out;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_put_records_subset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(mat), rs,
                       d_records, w32_rec, d_words, d_items, w32_out, n_records, bloom_size, n_colors_file, tail_mask(n_colors_file), d_err);
    return hipGetLastError();
}

// A workgroup's tile: about 8192 u32 words of records, at least one record and at most one per thread
hipError_t launch_put_records_folded(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, uint64_t n_records,
                                     const ModMagic &mod, hipStream_t stream) {
    if (n_records == 0) return hipSuccess;
    const uint64_t rpb = std::min<uint64_t>(kFoldBlock, std::max<uint64_t>(1, 8192u / record_words(w32_rec)));
    const uint64_t grid = (n_records + rpb - 1) / rpb;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;   // (a piece of stage_records is 256 MiB: at most 2^24 records)
    hipLaunchKernelGGL(k_put_records_folded, dim3((unsigned)grid), dim3(kFoldBlock), 0, stream, reinterpret_cast<uint32_t *>(mat), rs, d_records,
                       w32_rec, (uint32_t)rpb, n_records, mod);
    return hipGetLastError();
}

// Tiles of 64 records; a workgroup walks enough of them that about eight workgroups per CU exist — each flushes its counters once — and
// at most 2^16, the bound of the kernel's 32-bit LDS counters.  (A piece of stage_records is 256 MiB: at most 2^24 records, 2^18 tiles.)
hipError_t launch_put_records_grouped(GroupedParams p, int n_cu, hipStream_t stream) {
    if (p.n_records == 0) return hipSuccess;
    const uint32_t rws = (uint32_t)record_words(p.w32_rec) | 1u;
    p.staged = kWave * (uint64_t)rws <= kGroupTileWords ? 1u : 0u;
    const uint64_t n_tiles = (p.n_records + kWave - 1) / kWave;
    const uint64_t target = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
    const uint64_t tpb = std::min<uint64_t>(std::max<uint64_t>(1, (n_tiles + target - 1) / target), 1ull << 16);
    const uint64_t grid = (n_tiles + tpb - 1) / tpb;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    p.tiles_per_block = (uint32_t)tpb;
    const size_t shmem = p.staged ? 4ull * (kWave * rws + (p.counts ? 32u * (p.w32_rec + p.w32_out) : 0u)) : 0;   // <= 32 KiB + 2 * 128 * 121 B
    hipLaunchKernelGGL(k_put_records_grouped, dim3((unsigned)grid), dim3(kGroupBlock), shmem, stream, p);
    return hipGetLastError();
}

// About 2^20 threads at least: an output smaller than that takes its slices in several chunks (never more chunks than slices)
hipError_t launch_fold_rows(uint64_t *dst, const uint64_t *src, uint32_t rs, uint32_t w32, uint64_t m_dst, uint64_t factor, hipStream_t stream) {
    const uint64_t n = m_dst * w32;
    if (n == 0 || factor == 0) return hipSuccess;
    const uint64_t grid = (n + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t chunks = std::min<uint64_t>(std::min<uint64_t>(factor, 65535), std::max<uint64_t>(1, (1ull << 20) / n));
    hipLaunchKernelGGL(k_fold_rows, dim3((unsigned)grid, (unsigned)chunks), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(dst),
                       reinterpret_cast<const uint32_t *>(src), rs, w32, m_dst, factor);
    return hipGetLastError();
}

hipError_t launch_get_rows(const uint64_t *mat, uint32_t rs, const uint64_t *d_row_ids, uint32_t *d_words, uint32_t w32,
                           uint64_t n_rows, hipStream_t stream) {
    const uint64_t n = n_rows * w32;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_get_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint32_t *>(mat), rs, d_row_ids, d_words, w32, n_rows);
    return hipGetLastError();
}

hipError_t launch_insert_kmers(const InsertParams &p, hipStream_t stream) {
    const size_t shmem = (size_t)(kBlock / kWave) * (kmer_img_bytes(p.k) + (p.m_size ? kmer_img_bytes(p.m_size) : 0));
    const int grid = grid_for(p.n_kmers, p.tiles_per_block);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_insert_kmers, dim3(grid), dim3(kBlock), shmem, stream, p);
    return hipGetLastError();
}

}  // namespace cid
