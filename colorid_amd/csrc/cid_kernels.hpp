// Kernel parameter blocks and launchers shared by the kernel files (cid_search / cid_readid / cid_index .hip) and the ABI (cid_api_*.hip, cid_kmerset.hip).
#pragma once
#include "cid_device.hpp"

#include "cid_collapse.hpp"   // (after the HIP runtime: CID_HD)

namespace cid {

constexpr int kBlock = 256;  // 4 waves; every wave works on its own 64-k-mer tiles
#ifndef CID_READID_ALIAS
#define CID_READID_ALIAS 1   // k_readid: the search-phase histogram shares the hash table's LDS region (0: separate regions, A/B builds)
#endif
constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // a k-mer set built for an index: the sort key of a window without a k-mer (cid_partition.hpp, cid_windows.hpp)
constexpr int kPlanes = 8;   // bit-sliced per-colour counters per lane: drained every 255 k-mers

struct SearchParams {
    const uint64_t *mat;   // dense index, row r at mat + r*rs
    uint32_t rs;           // row stride in u64 words (1, or a power of two 2..128)
    uint32_t w64;          // words that carry colours = ceil(n_colors/64)
    uint32_t n_colors;
    uint32_t n_hash;
    uint32_t k;
    uint32_t c_pad;        // n_colors rounded up to even (LDS counter arrays)
    uint32_t wave_bytes;   // LDS bytes per wave: k-mer image + hash rows
    uint32_t want_unique;
    uint32_t tiles_per_block;  // block b owns tiles [b*tpb, (b+1)*tpb); grid = ceil(n_tiles/tpb)
    ModMagic mod;
    const uint8_t *kmers;  // n_kmers * k ASCII bytes, 16-byte aligned (or nullptr when codes != nullptr)
    const uint64_t *codes; // alternative input: canonical upper-case k-mers as 2-bit codes, base 0 most significant
    const uint32_t *freq;  // or nullptr
    uint64_t n_kmers;
    // a5 outputs (accumulated with atomics; caller zeroes)
    uint64_t *hits;
    uint64_t *n_unique;
    uint64_t *sum_unique_freq;
    uint32_t *unique_colour;
    // a4 outputs (caller presets and_words to all-ones, *missing to 0)
    uint64_t *and_words;
    int *missing;
    // colour-striped indices (this index holds colours [colour_base, colour_base + n_colors) of a wider one): the
    // per-k-mer facts that need every stripe are accumulated in caller-provided arrays instead of being decided here
    uint32_t colour_base;
    uint32_t *fact;        // [n_kmers] packed stripe fact, see stripe_fact_merge            (a5; nullptr = not striped)
    uint32_t *zero_acc;    // [n_kmers] &= bit s set iff row s is all-zero in this stripe  (a4; nullptr = not striped)
    // persistent, XCD-aware scheduling of k_search_count (nullptr = one contiguous tile range per block)
    uint32_t *queues;      // 8 work-queue heads, 32 words apart, zeroed before the launch
    int persist_grid;      // resident blocks: n_cu x blocks per CU
    uint32_t mixed;        // 32-byte rows: fetch each k-mer's last row through the scalar cache (gather_and_mixed32)
    uint32_t unroll;       // rows of >= 64 bytes: sub-passes whose loads are issued together (1 or 2)
};

struct InsertParams {
    uint64_t *mat;
    uint32_t rs;
    uint32_t n_hash;
    uint32_t k;
    uint32_t n_colors;
    uint32_t tiles_per_block;
    uint32_t colour;  // used when colour_of_kmer == nullptr
    uint32_t m_size;  // > 0: a minimizer (.mxi) index — the Bloom key is find_minimizer(kmer, m_size) (build.rs:455-459)
    ModMagic mod;
    const uint8_t *kmers;       // ASCII, or nullptr when codes != nullptr
    const uint64_t *codes;      // 2-bit canonical codes (k <= 32)
    const uint32_t *colour_of_kmer;
    uint64_t n_kmers;
};

struct ReadIdParams {
    const uint64_t *mat;
    uint32_t rs, w64, n_colors, n_hash, k;
    ModMagic mod;
    const uint8_t *bases;       // concatenated, quality-masked reads
    const uint64_t *seq_off;    // [n_seqs+1]
    const uint64_t *read_seq0;  // [n_reads+1]
    uint64_t n_reads;
    uint32_t stride_d, start_sample;
    uint32_t m_size;            // > 0: minimizer index — the per-read set holds minimizers (kmer.rs:363-394), hashed with length m_size
    uint32_t bases_cap;         // LDS bytes per wave for one read(-pair)'s bases (multiple of 16)
    uint32_t win_cap;           // max windows (= max distinct k-mers) of one read(-pair)
    uint32_t hist_pad;          // n_colors+1 rounded up to a multiple of 4
    uint32_t table_slots;       // power of two >= 1.5 x win_cap: the packed path's per-read k-mer set
    uint32_t idx_bits;          // > 0: one u64 per slot, code << idx_bits | first window index (2k + idx_bits <= 63; k_readid<..., PACKED>)
    uint32_t slot4;             // > 0: one u32 per slot, the earliest position of a window holding the slot's k-mer (k_readid<..., SLOT4>)
    uint32_t stage_bytes;       // k_readid: LDS bytes per wave for the next read's raw bases (multiple of 16, <= 1024; 0 = no read-ahead)
    uint32_t wave_bytes;        // LDS bytes per wave
    uint32_t reads_per_block;
    uint32_t *report;           // [n_reads][n_colors+1]
    uint32_t *n_kmers;          // [n_reads]
    uint8_t *status;            // [n_reads]
    const uint8_t *skip;        // NULL, or [n_reads]: non-zero = this read belongs to the sort-based path (k_readid_list), leave it alone
    uint32_t *redo_count;       // k_readid appends the reads it cannot pack (lower-case bases) to redo_list; k_readid_bytes
    uint32_t *redo_list;        //   works through that list (redo_list == NULL: through all reads, k > 32)
    // colour stripes (this index = colours [colour_base, colour_base + n_colors) of a wider one; all three NULL/0 otherwise).
    // "A row is absent" (read_id_mt_pe.rs:81-89, :126-128) means: all-zero in EVERY stripe, so the rule runs in two passes:
    //   zero pass  (zero_acc != NULL): every distinct k-mer of every read is looked up, nothing is counted;
    //              zero_acc[zero_start[read] + q] &= bit s set iff row s of the read's q-th k-mer is all-zero in this stripe
    //              (q = rank in the read's first-occurrence order — the same in the LDS kernels and in k_readid_list, so a read
    //              may take a different kernel in different stripes; zero_start = any prefix leaving >= windows(read) words per read);
    //   count pass (zero_in  != NULL): the ordered search, with "absent" read from the accumulated masks instead of this stripe's rows;
    //              report rows are report_width wide, this stripe's colours land at [colour_base ..), the no-hits entry at
    //              [report_width - 1] is written by the stripe with write_nohits set.
    uint32_t *zero_acc;
    const uint32_t *zero_in;
    const uint64_t *zero_start;   // [n_reads]
    uint32_t colour_base, report_width, write_nohits;
};

struct ReadIdListParams {  // k_readid_list: per-read distinct k-mers already in first-occurrence order
    const uint64_t *mat;
    uint32_t rs, w64, n_colors, n_hash, k;   // k = length of the listed keys (k-mers, or minimizers for a .mxi index)
    ModMagic mod;
    const uint64_t *list_codes;   // canonical 2-bit codes, base 0 most significant; with `bases`: key location << 1 | reverse-complement
    const uint8_t *bases;         // non-NULL: keys are byte strings inside `bases` (k > 32 or lower-case bases), k bytes each
    uint32_t upper;               // byte keys are upper-cased before hashing (.mxi minimizers)
    const uint64_t *list_start;   // [n_reads+1] offsets into list_codes
    uint64_t n_reads;
    uint32_t start_sample;
    uint32_t hist_pad, wave_bytes;
    uint32_t *report;
    uint32_t *n_kmers;
    const uint8_t *status;        // set by the caller: 1 = too_short, 2 = not this kernel's read (k_readid handles it)
    // colour stripes, as in ReadIdParams (all NULL/0: a whole index)
    uint32_t *zero_acc;
    const uint32_t *zero_in;
    const uint64_t *zero_start;
    uint32_t colour_base, report_width, write_nohits;
};

// The long-read path's in-order search (k_readid_slices): a read's ordered list of distinct k-mers is cut into slices of consecutive
// windows, one wave per slice; reads cut into several slices leave partial rows that k_readid_combine adds up in slice order.
struct ReadSlice {
    uint32_t read;
    uint32_t w0, w1;   // the slice's windows [w0, w1), numbered over the whole batch
    uint32_t part;     // index of the slice inside its read | 1 << 31 when the read has more than one slice
};
struct ReadCombine { uint32_t read, first_slice, n_slices, pad; };
struct ReadIdSliceParams {
    const uint64_t *mat;
    uint32_t rs, w64, n_colors, n_hash, k;   // k = length of the listed keys (k-mers, or minimizers for a .mxi index)
    ModMagic mod;
    const uint64_t *codes;        // every window's canonical 2-bit code (windows numbered over the batch; a read's start at a multiple of 32)
    const uint64_t *wstart, *wend;   // [n_reads]: a read's windows [wstart, wend)
    const uint32_t *bitmap;       // bit w: window w is the first occurrence of its k-mer in its read
    const uint32_t *word_prefix;  // exclusive prefix of the bitmap words' popcounts: rank(w) = word_prefix[w >> 5] + popc(bits below w)
    const ReadSlice *slices;
    uint32_t n_slices;
    uint32_t start_sample;
    uint32_t hist_pad, wave_bytes;
    uint32_t *report;
    uint32_t *n_kmers;
    uint32_t *partial;            // [n_slices][n_colors + 2]: counts | no-hits | stopped — only rows of multi-slice reads are written
    // soft-masked reads (k_long_bytes): bytes_read[r] != 0 — read r's entries in `codes` are (byte offset in bases << 1 | reverse complement)
    // of byte-string k-mers; the plain kernel leaves those reads to the BYTES instantiation and the other way round.  NULL: no such reads
    const uint8_t *bytes_read;
    const uint8_t *bases;
};
hipError_t launch_readid_slices(const ReadIdSliceParams &p, int grid, hipStream_t stream, bool bytes = false);
hipError_t launch_readid_combine(const ReadCombine *d_comb, uint32_t n_comb, const uint32_t *d_partial, uint32_t n_colors, uint32_t *d_report,
                                 hipStream_t stream);

size_t search_smem_bytes(const SearchParams &p);
hipError_t launch_readid_list(const ReadIdListParams &p, int grid, hipStream_t stream);
hipError_t launch_readid(const ReadIdParams &p, int waves_per_block, hipStream_t stream);
hipError_t launch_readid_bytes(const ReadIdParams &p, int waves_per_block, int grid, hipStream_t stream);
hipError_t launch_readid_check_caps(const ReadIdParams &p, uint8_t *skip, hipStream_t stream);
hipError_t launch_unique_finalize(const uint32_t *fact, const uint32_t *freq, uint64_t n_kmers,
                                  uint32_t n_colors_total, uint64_t *n_unique, uint64_t *sum_unique_freq, uint32_t *unique_colour,
                                  hipStream_t stream);
int grid_for(uint64_t n_kmers, uint32_t tiles_per_block);
hipError_t launch_search_count(const SearchParams &p, hipStream_t stream);
int search_count_blocks_per_cu(const SearchParams &p);
hipError_t launch_search_perfect(const SearchParams &p, hipStream_t stream);
// Segmented search (cid_segments.hip): segment s = k-mers [seg_off[s], seg_off[s+1]) of s.kmers; hits[s * n_colors + c] and missing[s]
// are added to / set (caller zeroes).  Of `s` the a5 / a4 outputs and the stripe fields are unused; rows of at most 128 words.
struct SegmentParams {
    SearchParams s;
    const uint64_t *seg_off;   // [n_segs + 1], non-decreasing, seg_off[0] = 0, seg_off[n_segs] = s.n_kmers
    uint64_t n_segs;           // < 2^32
    uint32_t *hits;            // [n_segs][n_colors]
    uint8_t *missing;          // [n_segs], or nullptr
};
hipError_t launch_search_segments(const SegmentParams &p, hipStream_t stream);
// Segmented perfect search (cid_perfect_segments.hip): and_words[s * s.rs + w] is ANDed with the rows of segment s's k-mers and missing[s]
// set (caller presets all ones / 0); k_perfect_segments_finish then zeroes the words of empty and flagged segments and the bits past the
// last colour.  Of `s` only the index, the k-mers, wave_bytes (perfect_segments_wave_bytes; c_pad = 0) and tiles_per_block are used.
struct PerfectSegmentParams {
    SearchParams s;
    const uint64_t *seg_off;   // [n_segs + 1], non-decreasing, seg_off[0] = 0, seg_off[n_segs] = s.n_kmers
    uint64_t n_segs;           // < 2^32
    uint64_t *and_words;       // [n_segs][s.rs]
    uint8_t *missing;          // [n_segs], never null
};
size_t perfect_segments_wave_bytes(uint32_t k, uint32_t n_hash);
hipError_t launch_perfect_segments(const PerfectSegmentParams &p, hipStream_t stream);
// seg_off: the segments' TRUE offsets (a host-form launch sees clipped ones); only the differences are read
hipError_t launch_perfect_segments_finish(uint64_t *and_words, const uint8_t *missing, const uint64_t *seg_off, uint64_t n_segs, uint32_t rs,
                                          uint32_t n_colors, hipStream_t stream);
// Nearest-allele reduction (cid_nearest.hip): k_search_segments' counters of the segments [s_lo, s_hi) -> per (group, colour) the segment
// with the largest share, MERGED into out (caller presets: launch_nearest_preset).  Group g of the launch = segments
// [group_off[g], group_off[g + 1]) clipped to [s_lo, s_hi); segment numbers are those group_off speaks of.
constexpr int kNearestGroups = 4;   // consecutive groups per workgroup: one per wave in the final merge
struct NearestParams {
    const uint32_t *hits;        // row of segment s at hits + (s - s_lo) * n_colors
    const uint64_t *seg_off;     // [s_hi - s_lo + 1]: entry s - s_lo; only the differences are read
    const uint64_t *group_off;   // [n_groups + 1], the launch's first group first
    uint64_t n_groups;           // of this launch; < 2^33
    uint64_t g_base;             // the launch's first group's row of `out`
    uint64_t s_lo, s_hi;
    uint32_t n_colors;
    uint4 *out;                  // [.][n_colors] cells {seg, kmers_hit, n_kmers, n_perfect}
};
hipError_t launch_nearest_groups(const NearestParams &p, hipStream_t stream);
hipError_t launch_nearest_preset(void *out, uint64_t n_cells, hipStream_t stream);
// Coverage search (cid_cover.hip): the segmented search with the windows kept in order.  k_cover_rows writes every window's AND words to
// rows[window * s.rs + word] (zeros for a window whose flag byte lacks bit 0); k_cover_stats turns the bits of segment s = windows
// [seg_off[s], seg_off[s+1]) into out[s * n_colors + c], eight u32 per cell (include/colorid_hip.h: cid_cover).  Of `s` only the index,
// the k-mers, wave_bytes (image + hash rows; c_pad = 0) and tiles_per_block are used; rows of at most 128 words.
struct CoverParams {
    SearchParams s;
    const uint8_t *flags;      // [s.n_kmers] bit 0 = the window holds a k-mer, bit 1 = first window of its segment with that k-mer; or nullptr = 3 everywhere
    uint64_t *rows;            // [s.n_kmers][s.rs]
    const uint64_t *seg_off;   // [n_segs + 1], non-decreasing, seg_off[n_segs] <= s.n_kmers
    uint64_t n_segs;           // n_segs * s.w64 < 2^33
    uint32_t *out;             // [n_segs][n_colors][8]
};
hipError_t launch_cover_rows(const CoverParams &p, hipStream_t stream);
hipError_t launch_cover_stats(const CoverParams &p, hipStream_t stream);
// Greedy cover of a query by accessions (cid_gather_cover.hip; include/colorid_hip.h: cid_search_gather) over k_cover_rows' matrix.
// GatherRound is the state the rounds share, all of it on the device; the host reads its first 16 bytes once a round.
struct GatherRound {
    uint32_t stop;                    // set by k_gather_pick: this round emits nothing and there is no next one
    uint32_t colour;                  // the round's pick (bounded by n_colors wherever it is read back)
    uint64_t n_out;                   // rows emitted so far
    unsigned long long live, n_hit;   // k-mers not yet explained; k-mers with a colour at all
};
struct GatherParams {
    const uint64_t *rows;          // [n_kmers][rs]
    const uint32_t *freq;          // [n_kmers] or nullptr = 1 everywhere
    uint64_t n_kmers;
    uint32_t rs, w64, n_colors;
    uint32_t tiles_per_wave;       // k_gather_mark, k_gather_fold: consecutive 64-row tiles of one wave
    uint64_t *alive;               // [ceil(n_kmers / 64)] bit l of word t: row 64t + l is live and has a colour
    uint64_t *removed;             // [ceil(n_kmers / 64)] the rows the round's pick takes out
    unsigned long long *cnt_new;   // [n_colors] new_t[c]
    unsigned long long *total, *total_weight;   // [n_colors]
    GatherRound *round;
    void *out;                     // [max_rows] cid_gather_row
    uint64_t min_new, max_rows;
};
hipError_t launch_gather_init(const GatherParams &p, hipStream_t stream);     // alive, n_hit, live
hipError_t launch_gather_totals(const GatherParams &p, hipStream_t stream);   // total, total_weight (added to: caller zeroes)
hipError_t launch_gather_pick(const GatherParams &p, hipStream_t stream);     // arg-max of cnt_new -> a row, or stop
hipError_t launch_gather_round(const GatherParams &p, hipStream_t stream);    // mark the pick's rows, subtract their bits from cnt_new
hipError_t launch_put_rows(uint64_t *mat, uint32_t rs, const uint64_t *d_row_ids, const uint32_t *d_words, uint32_t w32,
                           uint64_t n_rows, hipStream_t stream);
hipError_t launch_put_records(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, uint32_t w_off, uint32_t w32_take,
                              uint64_t n_records, uint64_t bloom_size, uint32_t n_colors, uint32_t *d_err, hipStream_t stream);
// One output word that the colours of a merged file reach: the file colours [lo, lo + popc(mask)) become the set bits of `mask`
// in u32 word w of every row (k_put_records_mapped).
struct MergePlan { uint32_t w, lo, mask, pad; };
hipError_t launch_put_records_mapped(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, const MergePlan *d_plan,
                                     uint32_t n_plan, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors_file, uint32_t *d_err,
                                     hipStream_t stream);
// `subset`: the plan of an extraction of kept colours (k_put_records_subset).  Items: the file words that keep anything, ascending.
// Per output u32 word j: kept bits 32j .. 32j+31 of a row lie in items [first, first + n_items); `skip` kept bits of item `first`
// belong to earlier output words.
struct SubsetItem { uint32_t s, mask; };
struct SubsetWord { uint32_t first, skip, n_items, pad; };
hipError_t launch_put_records_subset(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, const SubsetWord *d_words,
                                     const SubsetItem *d_items, uint32_t w32_out, uint64_t n_records, uint64_t bloom_size,
                                     uint32_t n_colors_file, uint32_t *d_err, hipStream_t stream);
// `fold`: checked records of a file whose Bloom size is a multiple of mod.m, OR-ed into row (record's row) % mod.m (k_put_records_folded);
// and the rows of a resident matrix of factor * m_dst rows with the same row stride, OR-ed into dst's row % m_dst (k_fold_rows).
hipError_t launch_put_records_folded(uint64_t *mat, uint32_t rs, const uint32_t *d_records, uint32_t w32_rec, uint64_t n_records,
                                     const ModMagic &mod, hipStream_t stream);
hipError_t launch_fold_rows(uint64_t *dst, const uint64_t *src, uint32_t rs, uint32_t w32, uint64_t m_dst, uint64_t factor, hipStream_t stream);
// `collapse`: checked records of a file with n_colors_file colours through the many-to-one plan of cid_collapse.hpp into the index's
// n_colors colours, rows stored (k_put_records_grouped).  counts: n_colors_file + n_colors u64 counters that the records with a file
// colour / an output colour set are ADDED to, or nullptr.  The launcher fills in tiles_per_block and staged; n_cu sizes the grid.
struct GroupedParams {
    uint32_t *mat32;
    uint32_t rs;
    const uint32_t *rec32;
    uint32_t w32_rec, w32_out, n_colors_file, n_colors;
    const GroupWord *words;
    const GroupItem *items;
    uint64_t n_records;
    uint32_t tiles_per_block, staged;
    unsigned long long *counts;
};
hipError_t launch_put_records_grouped(GroupedParams p, int n_cu, hipStream_t stream);
// `compare`: shared[i][j] += popcount(column i & column j) over the rows of one source (k_pairs).  The rows are w32 u32 words at
// rows + row*stride + off (u32 units): a chunk of file records (stride 6 + w32, off 4) or a resident index's matrix (stride 2*rs, off 0).
// shared: n_colors x n_colors u64 counters, row-major; only i <= j is added to.  The launcher fills in the grid fields.
struct PairsParams {
    const uint32_t *rows;
    uint64_t stride;
    uint32_t off, w32;
    uint64_t n_rows;
    uint32_t n_colors;
    unsigned long long *shared;
    uint32_t n_blocks, n_pair_groups, tiles_per_block;   // 64-colour blocks; groups of four block pairs; row tiles per workgroup
    uint64_t n_pairs, chunk0;                            // block pairs I <= J; the launch's first row chunk
};
hipError_t launch_pairs_check(const uint32_t *d_records, uint32_t w32_rec, uint64_t n_records, uint64_t bloom_size, uint32_t n_colors,
                              uint32_t *d_err, hipStream_t stream);
hipError_t launch_pairs(PairsParams p, int n_cu, hipStream_t stream);
// `dists`: the allele distances of a cgMLST table (cid_dists.hip).  T: the codes transposed, L rows of Ap u32 (Ap = A rounded up to 64, the
// padding zero); maskT: W = ceil(L / 64) rows of Ap u64, the called-loci bitmasks.  launch_dists_put deposits the accessions [a0, a0 + na)
// of a row-major piece into both and ORs 1 into *d_err for a code of 0xFFFFFFFE or 0xFFFFFFFF.  launch_dists_tile fills the rows [row0,
// row0 + n_rows) of differ and (unless null) compared, each n_rows x A u32; at most kDistsMaxRowTiles tiles of 64 rows a launch.
struct DistsParams {
    const uint32_t *T;
    const unsigned long long *maskT;
    uint64_t Ap;
    uint32_t A, L, W, row0, n_rows;
    uint32_t *differ, *compared;
};
constexpr uint32_t kDistsMaxRowTiles = 65535;
hipError_t launch_dists_put(const uint32_t *d_codes, uint32_t a0, uint32_t na, uint32_t L, uint32_t *T, unsigned long long *maskT, uint64_t Ap,
                            uint32_t *d_err, hipStream_t stream);
hipError_t launch_dists_tile(const DistsParams &p, hipStream_t stream);
// One Borůvka round over the same arrays (p's row0, n_rows, differ and compared are not read): for every accession i, best[i] = the least
// key = differ << shift_differ | (L - compared) << shift_compared | j over the j with comp[j] != comp[i] and compared(i, j) >=
// min_compared (>= 1), or kDistsNoBest.  launch_dists_best presets best and fills in the shifts; dists_best_shifts gives them for a shape
// and says whether the key fits 64 bits: 2 ceil(log2(L + 1)) + ceil(log2 A) <= 64 (else the launcher returns hipErrorInvalidValue).
struct DistsBestParams {
    const uint32_t *comp;        // [A] component labels, any u32
    unsigned long long *best;    // [A]
    uint32_t min_compared, shift_differ, shift_compared;
};
constexpr unsigned long long kDistsNoBest = ~0ull;
bool dists_best_shifts(uint32_t A, uint32_t L, uint32_t *shift_differ, uint32_t *shift_compared);
hipError_t launch_dists_best(DistsParams p, DistsBestParams b, hipStream_t stream);
// The neighbour list over the same arrays (p's differ and compared are not read): every pair (i in [row0, row0 + n_rows), j < A, j != i)
// with compared >= min_compared (>= 1) and differ <= max_differ — upper: also j > i — is appended to list as {i, j, differ, compared},
// its slot taken from *cursor, which the caller has set to 0.  Entries at or past cap are not stored and still counted: after the launch
// *cursor is the number of hits (cap = 0: a count, list may be null).  The order inside list is the order of the atomics: sort it.
// At most kDistsMaxRowTiles tiles of 64 rows a launch.
struct DistsWithinParams {
    uint4 *list;                   // [cap] entries a, b, differ, compared
    unsigned long long cap;
    unsigned long long *cursor;
    uint32_t max_differ, min_compared, upper;
};
hipError_t launch_dists_within(const DistsParams &p, const DistsWithinParams &w, hipStream_t stream);
// The K nearest over the same arrays (p's differ and compared are not read): for every row i of [row0, row0 + n_rows) and every column
// tile t, part[((i - row0) * (Ap / 64) + t) * k + n] = the n-th least key (k_dists_best's, the same shifts: the launcher fills them in) over
// the tile's columns j != i, j < A with compared >= min_compared (>= 1) and differ <= max_differ, or kDistsNoBest past the last of them.
// Every one of those slots is written: part needs no preset.  1 <= k <= kDistsClosestMax; at most kDistsMaxRowTiles tiles of 64 rows a
// launch.  launch_dists_closest_merge: one level of the merge — per row n_lists such lists of k keys in, ceil(n_lists / 64) out, list g
// the k least keys of the lists [64 g, 64 g + 64) in order; repeated until one list a row is left, that is the row's k nearest.
constexpr uint32_t kDistsClosestMax = 64;   // CID_DISTS_CLOSEST_MAX; no more than a tile's 64 columns: a tile's list is k long, not min(k, 64)
struct DistsClosestParams {
    unsigned long long *part;      // [n_rows][Ap / 64][k]
    uint32_t k, max_differ, min_compared, shift_differ, shift_compared;
};
hipError_t launch_dists_closest(const DistsParams &p, DistsClosestParams q, hipStream_t stream);
hipError_t launch_dists_closest_merge(const unsigned long long *in, unsigned long long *out, uint64_t n_rows, uint64_t n_lists, uint32_t k,
                                      hipStream_t stream);
// The two histograms over the same arrays (p's differ and compared are not read): every pair (i in [row0, row0 + n_rows), j < A, j != i)
// — upper: also j > i — adds 1 to compared_hist[compared] and, when compared >= min_compared (>= 1), 1 to differ_hist[differ]; both are
// L + 1 u64 that the caller has set to 0.  Any number of rows a launch: the grid is one-dimensional, at most kDistsHistBlocksPerCu
// workgroups a CU (n_cu: the device's), each with a contiguous share of the tiles that hold a pair — in upper mode those not wholly on
// or below the diagonal — of at most kDistsHistMaxShare tiles: with more tiles than that the grid grows instead.
struct DistsHistParams {
    unsigned long long *differ_hist, *compared_hist;   // [L + 1] each
    uint32_t min_compared, upper;
    uint64_t n_tiles;                                  // (filled in by the launcher)
};
constexpr uint32_t kDistsHistWindow = 4096;            // bins 0 .. 4095 of either histogram are counted in LDS, the bins above in place
constexpr uint32_t kDistsHistBlocksPerCu = 3;          // what 16 KiB of walk + 2 x 16 KiB of bins leave room for in a CU's 160 KiB of LDS
constexpr uint64_t kDistsHistMaxShare = 0xFFFFFFFFull / (64 * 64);   // tiles a workgroup may own: 4 096 pairs a tile and no u32 bin wraps
hipError_t launch_dists_hist(const DistsParams &p, DistsHistParams h, int n_cu, hipStream_t stream);
hipError_t launch_get_rows(const uint64_t *mat, uint32_t rs, const uint64_t *d_row_ids, uint32_t *d_words, uint32_t w32,
                           uint64_t n_rows, hipStream_t stream);
hipError_t launch_insert_kmers(const InsertParams &p, hipStream_t stream);

}  // namespace cid
