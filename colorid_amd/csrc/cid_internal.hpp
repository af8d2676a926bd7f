// Internals shared by the translation units of libcolorid_hip.so (not part of the ABI).
#pragma once
#include <vector>
#include "cid_kernels.hpp"
#include "cid_readbatch.hpp"

struct cid_ctx;
struct cid_index;
struct cid_kmerset;

namespace cid {

int fail(int code, const char *fmt, ...);  // records the thread's last error message, returns `code`
int ctx_device(const cid_ctx *c);
hipStream_t ctx_stream(const cid_ctx *c);
int ctx_order_bits(const cid_ctx *c);
int ctx_n_cu(const cid_ctx *c);
// the ctx's own stream, its second (copy) stream and two untimed events for calls that overlap an upload with kernels; free between calls
hipStream_t ctx_own_stream(const cid_ctx *c);
hipStream_t ctx_copy_stream(const cid_ctx *c);
hipEvent_t ctx_event(const cid_ctx *c, int i);   // cid_ctx_tune "order_bits"
// Device scratch that survives the call: hipMalloc of a GiB-sized block costs tens of milliseconds here (the driver clears
// it), so blocks go back to a per-ctx cache instead of hipFree and the next batch takes them again.  All users run on the
// ctx stream, which orders a block's last kernel before its next owner's first.  Objects holding such blocks
// (cid_kmerset, sparse read_id results) must be destroyed before their ctx.
int ctx_alloc(cid_ctx *c, size_t bytes, void **out);
void ctx_free(cid_ctx *c, void *p);
uint32_t kmerset_k(const cid_kmerset *ks);
cid_ctx *kmerset_ctx(const cid_kmerset *ks);
uint32_t index_k(const cid_index *ix);
uint32_t index_rs(const cid_index *ix);
ModMagic index_mod(const cid_index *ix);
uint32_t index_n_colors(const cid_index *ix);
uint32_t index_n_hash(const cid_index *ix);
uint32_t index_m_size(const cid_index *ix);
const uint64_t *index_matrix(const cid_index *ix);

// contiguous, balanced partition (the same rule as colorid_amd/dist.py shard_bounds): sizes differ by at most one
inline void shard_bounds(size_t n_units, int rank, int world, size_t *lo, size_t *hi) {
    const size_t base = n_units / (size_t)world, rem = n_units % (size_t)world;
    *lo = (size_t)rank * base + ((size_t)rank < rem ? (size_t)rank : rem);
    *hi = *lo + base + ((size_t)rank < rem ? 1 : 0);
}

// the same with every boundary on a multiple of 64 units (byte-string k-mers: a shard's first k-mer must sit on a 16-byte boundary)
inline void shard_bounds64(size_t n_units, int rank, int world, size_t *lo, size_t *hi) {
    const size_t blocks = (n_units + 63) / 64;
    shard_bounds(blocks, rank, world, lo, hi);
    *lo *= 64; *hi *= 64;
    if (*lo > n_units) *lo = n_units;
    if (*hi > n_units) *hi = n_units;
}

// k-mers on a device, in one of their two encodings: byte strings (any k; the only form for k > 32) or 2-bit codes (k <= 32).
// A view: it owns nothing.
struct DevKeys {
    const uint8_t *ascii = nullptr;     // n x k bytes, 16-byte aligned
    const uint64_t *codes = nullptr;    // n codes; exactly one of the two is set when n > 0
    const uint32_t *counts = nullptr;   // multiplicities, or NULL
    size_t n = 0;
    uint32_t k = 0;
    cid_ctx *ctx = nullptr;             // whose memory this is; NULL for a caller's device pointers
    size_t unit() const { return ascii ? k : 8; }   // bytes per key
    const uint8_t *bytes() const { return ascii ? ascii : reinterpret_cast<const uint8_t *>(codes); }
    DevKeys slice(size_t lo, size_t hi) const {     // keys [lo, hi)
        DevKeys s = *this;
        if (ascii) s.ascii += lo * k;
        if (codes) s.codes += lo;
        if (counts) s.counts += lo;
        s.n = hi - lo;
        return s;
    }
    // rank's share of `world` contiguous ones; byte strings in blocks of 64 keys: a shard's first byte must sit on a 16-byte boundary
    void shard(int rank, int world, size_t *lo, size_t *hi) const {
        if (ascii) shard_bounds64(n, rank, world, lo, hi); else shard_bounds(n, rank, world, lo, hi);
    }
};

// a finalized set's device arrays (codes ascending unless reordered, byte strings for k > 32; counts u32), keys->ctx the ctx they live in
int kmerset_keys(const cid_kmerset *ks, DevKeys *keys);
// Bloom insert of k-mers already on the device into one colour (build.rs:62-66 with the k-mer map on the GPU); waits for the stream
int index_insert_keys(cid_index *ix, const DevKeys &keys, uint32_t colour);
// a5 launch on device-resident inputs/outputs (zeroes the counters first); asynchronous on the ctx stream
int search_count_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *d_hits, uint64_t *d_n_unique, uint64_t *d_sum_unique_freq,
                        uint32_t *d_unique_colour, bool zero_counters = true);
// a4 launch: d_and (rs words) and d_missing (int) are preset here; asynchronous
int search_perfect_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *d_and, int *d_missing);
// k_cover_rows on keys of either encoding: every key's AND words to d_rows[key * row stride + word] (d_flags: cid_search_cover's, or NULL);
// asynchronous on the ctx stream, the caller has checked the index (at most 8192 colours, no minimizers) and set the device
int cover_rows_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, const uint8_t *d_flags, uint64_t *d_rows);
// a5 / a4 on k-mers that are already on the device (keys.k must be the index's); outputs go to HOST buffers
int search_count_keys(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *hits, uint64_t *n_unique, uint64_t *sum_unique_freq,
                      uint32_t *unique_colour);
int search_perfect_keys(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint32_t *and_words_le, int *any_row_missing);

// read_id over colour stripes (ReadIdParams::zero_acc ...): which pass this launch is, and where its results go; all zero = a whole index
struct StripePass {
    uint32_t *zero_acc = nullptr;
    const uint32_t *zero_in = nullptr;
    const uint64_t *zero_start = nullptr;   // device, [n_reads]
    uint32_t colour_base = 0, report_width = 0, write_nohits = 0;
    bool on() const { return zero_acc || zero_in; }
};

// a batch of reads on a device (bases AND offsets), and the device arrays a read_id launch leaves its results in
struct DevReads {
    const uint8_t *d_bases = nullptr;
    const uint64_t *d_seq_off = nullptr, *d_read_seq0 = nullptr;
    size_t n_reads = 0;
    uint32_t stride_d = 1, start_sample = 0;
};
struct ReadOut { uint32_t *d_report = nullptr, *d_n_kmers = nullptr; uint8_t *d_status = nullptr; };

// read_id for reads that do not fit (or badly fit) a wave's LDS (cid_readlong.hip): per-read k-mer sets by workgroup-wide LDS hash
// tables, the ordered search by slices of a read.  Everything — bases AND offsets — is on the device; the work lists are made there
// (round 6).  d_route == NULL: every read; else only reads with d_route[r] == 1 — the others get status 2 and nothing else is written
// for them.  clear_wide: zero the whole report first when rows are wider than 128 words (those kernels count in place).  host: the
// same offsets on the host when the caller has them (NULL: downloaded IF a read needs the sorting path).
// d_route_stats (4 words, long_route_launch's) come down into route_stats with the plan's totals.  Waits for the stream twice: for the
// lists' sizes (64 bytes) before its kernels, and at its end.
int readid_long(cid_ctx *c, const cid_index *ix, const DevReads &b, const uint8_t *d_route, bool clear_wide, const ReadOut &o,
                const StripePass &sp = StripePass(), const HostOffsets *host = nullptr, const uint32_t *d_route_stats = nullptr,
                uint32_t *route_stats = nullptr);
// d_route[r] = 1: read r has at least long_from bases (the long-read path's), 0: the LDS kernels', 3: beyond cap_bytes / cap_win (what a
// device-pointer caller stated as maxima; long_beyond_launch gives those status 3 and an empty row).  d_stats[4]: long reads, LDS-kernel
// reads, the longest of the latter in bases and in windows.  Asynchronous.
int long_route_launch(cid_ctx *c, const DevReads &b, uint32_t k, uint64_t long_from, uint64_t cap_bytes, uint64_t cap_win, uint8_t *d_route,
                      uint32_t *d_stats);
int long_beyond_launch(cid_ctx *c, const uint8_t *d_route, size_t n_reads, uint32_t report_width, const ReadOut &o);
// the same by a global radix sort of every window of the batch (cid_kmerset_cold.hip; round 1's path): byte-string keys — k > 32, or the
// reads with a lower-case base that readid_long hands back (merge_status: only the routed reads' statuses are written).  Of b the bases are
// read on the device; the offsets are host's.
int readid_long_sorted(cid_ctx *c, const cid_index *ix, const DevReads &b, const HostOffsets &host, const uint8_t *route, bool clear_wide,
                       const ReadOut &o, const StripePass &sp = StripePass(), bool merge_status = false);

// rocPRIM behind plain calls (cid_kmerset_cold.hip — the one translation unit that includes it; its code object of some thousand kernels is
// loaded when the first of these is called): stable LSD radix sorts on bits [b0, b1), a run-length count of sorted keys.  Asynchronous on `st`.
int cold_sort_keys_u64(cid_ctx *c, hipStream_t st, const uint64_t *in, uint64_t *out, size_t n, unsigned b0, unsigned b1);
int cold_sort_pairs_u64_u32(cid_ctx *c, hipStream_t st, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned b0,
                            unsigned b1);
int cold_sort_pairs_u32_u64(cid_ctx *c, hipStream_t st, const uint32_t *kin, uint32_t *kout, const uint64_t *vin, uint64_t *vout, size_t n, unsigned b0,
                            unsigned b1);
int cold_run_length_u64(cid_ctx *c, hipStream_t st, const uint64_t *sorted, size_t n, uint64_t *uniq, uint32_t *runs, uint64_t *d_n_runs);

// replace a finalized 2-bit-code set's contents by the merge (sort by code, add counts of equal codes) of `total` pairs on its device
int kmerset_assign_merged(cid_kmerset *ks, const uint64_t *d_codes_in, const uint32_t *d_counts_in, size_t total);
// d_modes[c] = the most frequent multiplicity among the k-mers whose unique colour is c (ties -> the smallest; 0 = none); asynchronous
int unique_freq_modes(cid_ctx *c, const uint32_t *d_uc, const uint32_t *d_freq, uint64_t n, uint32_t C, uint64_t *d_modes);
// the same in two asynchronous steps (cid_reports.hip): after _begin d_modes holds the modes over the multiplicities below the table's
// width and w->ovf_count[0] (device) the number of k-mers beyond it; _finish counts those in when there are any and frees w's arrays
struct ModeWork {
    uint64_t *ovf = nullptr;
    unsigned long long *best = nullptr, *ovf_count = nullptr;
    uint32_t C = 0;
};
int unique_freq_modes_begin(cid_ctx *c, const uint32_t *d_uc, const uint32_t *d_freq, uint64_t n, uint32_t C, uint64_t *d_modes, ModeWork *w);
int unique_freq_modes_finish(cid_ctx *c, ModeWork *w, unsigned long long n_ovf, uint64_t *d_modes);
// sorted (colour << 32 | multiplicity) keys and their k-mer counts over the k-mers with a unique colour (host vectors; synchronous)
int unique_freq_hist(cid_ctx *c, const uint32_t *d_uc, const uint32_t *d_freq, uint64_t n, std::vector<uint64_t> &keys, std::vector<uint32_t> &counts);

// the non-zero rows of [row_begin, row_begin + n_rows) as .bxi row records in a host buffer (cid_kmerset.hip)
int index_get_records(cid_ctx *c, const cid_index *ix, uint64_t row_begin, uint64_t n_rows, uint8_t *records, uint64_t *n_records);

// dense report rows (device) -> per-row (colour, count) lists, ascending colour; outputs are ctx_alloc'ed for the caller (return them with ctx_free)
int compact_report(cid_ctx *c, const uint32_t *d_report, uint32_t width, uint64_t n_rows, uint64_t **d_row_start, uint32_t **d_colours,
                   uint32_t **d_counts, uint64_t *n_entries);
// ... as the ctx's sparse result (what cid_readid_sparse_fetch hands out), in place of the one it held
int store_sparse(cid_ctx *c, const uint32_t *d_report, uint32_t width, uint64_t n_rows);

// block-gzip members on the device (cid_inflate.hip): member i = in[in_off, +in_len) (header, DEFLATE data, CRC-32, ISIZE), its text to
// out[out_off, +out_len); status[i] = 0 or the reason it is corrupt.  Asynchronous on `stream`.
struct BgzfMember { uint32_t in_off, in_len, out_off, out_len; };
// d_scratch: bgzf_inflate_scratch_bytes(n_members) bytes the launch may use until it has run (match tokens of the wave-parallel kernel, its
// retry list), or NULL (one lane per member)
size_t bgzf_inflate_scratch_bytes(uint32_t n_members);
hipError_t bgzf_inflate_launch(cid_ctx *c, hipStream_t stream, const uint8_t *d_in, const BgzfMember *d_mem, uint32_t n_members, uint8_t *d_out,
                               uint32_t *d_st, void *d_scratch);
const char *bgzf_status_text(uint32_t st);

// load a translation unit's code object ahead of its first kernel launch (cid_warmup)
hipError_t warm_readid();
hipError_t warm_readlong();
hipError_t warm_cold();
hipError_t warm_search();
hipError_t warm_kmerset();
hipError_t warm_reports();
hipError_t warm_inflate();
hipError_t warm_fastq();
hipError_t warm_deflate();
// the text at d_text (16-byte aligned) as block-gzip members back to back at d_members (cid_bgzf_deflate_bound bytes of room), their lengths and
// *d_total = their bytes; queued on `stream`, which must be the stream the ctx's block cache is ordered on (c->stream)
int bgzf_deflate_launch(cid_ctx *c, hipStream_t stream, const uint8_t *d_text, size_t text_bytes, uint8_t *d_members, uint32_t *d_member_len, uint64_t *d_total,
                        bool matches = false);   // matches: with LZ77 matches (cid_bgzf_deflate_lz)
// The segmented form (cid_bgzf_deflate_segments, cid_fastq_split): n_segs texts in one buffer, each cut every 65 280 bytes from its own start.
// _layout: d_seg_len [n_segs] -> d_base [n_segs + 1] (segment s's text at d_text + base[s], the lengths rounded up to 16; element n_segs =
// the room the texts take) and d_piece_first [n_segs + 1] (the index of s's first piece; element n_segs = the pieces).  _launch: the
// n_pieces members back to back at d_members (text room + 31 per piece), their lengths, *d_total, and (d_seg_off [n_segs + 1], may be null)
// where each segment's members begin.  Same stream rule as bgzf_deflate_launch.
int bgzf_segments_layout(cid_ctx *c, hipStream_t stream, const uint64_t *d_seg_len, size_t n_segs, uint64_t *d_base, uint64_t *d_piece_first);
int bgzf_deflate_segments_launch(cid_ctx *c, hipStream_t stream, const uint8_t *d_text, const uint64_t *d_seg_len, const uint64_t *d_base,
                                 const uint64_t *d_piece_first, size_t n_segs, size_t n_pieces, uint8_t *d_members, uint32_t *d_member_len, uint64_t *d_total,
                                 uint64_t *d_seg_off, bool matches);
hipError_t ctx_side_streams(cid_ctx *c, hipStream_t out[4]);   // created on first use; any thread

}  // namespace cid
