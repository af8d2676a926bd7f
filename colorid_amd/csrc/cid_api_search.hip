// C ABI of libcolorid_hip.so, part 3: the searches — a5 proportional (src/batch_search_pe.rs:45-84, :125-164) and a4 perfect
// (src/perfect_search.rs:25-52, :83-110), whole indices and colour stripes, device-pointer and host-pointer forms — and the searches
// over many segments a call: counters, perfect, nearest per group (one host walk for the three: walk_segments, cid_segplan.hpp), coverage.
// Kernels: cid_search.hip, cid_segments.hip, cid_perfect_segments.hip, cid_nearest.hip, cid_cover.hip.
#include "cid_api_common.hpp"
#include "cid_segplan.hpp"

using cid::aligned16;
using cid::check_not_mini;
using cid::check_ready;
using cid::fail;
using cid::pick_tiles_per_block;
using cid::slot_reserve;
using cid::upload_chunk_kmers;
using namespace cid::slots;

namespace {

// the index's search parameters with `keys` as the query (outputs and modes are the caller's to set); refuses keys that no kernel can read
int fill_search_params(const cid_ctx *c, const cid_index *ix, const cid::DevKeys &keys, cid::SearchParams &p) {
    if (keys.n && !keys.ascii && !keys.codes) return fail(CID_ERR_INVALID, "null argument");
    if (keys.ascii && !aligned16(keys.ascii)) return fail(CID_ERR_INVALID, "d_kmers must be 16-byte aligned");
    if (keys.codes && ix->k > 32) return fail(CID_ERR_UNSUPPORTED, "2-bit codes need k_size <= 32");
    memset(&p, 0, sizeof(p));
    p.mat = ix->mat;
    p.rs = ix->rs;
    p.w64 = ix->w64;
    p.n_colors = ix->n_colors;
    p.n_hash = ix->n_hash;
    p.k = ix->k;
    p.c_pad = (ix->n_colors + 1u) & ~1u;
    if (p.c_pad < 2) p.c_pad = 2;
    p.wave_bytes = cid::kmer_img_bytes(ix->k) + cid::kWave * ix->n_hash * 4u + 2u * cid::kWave * 4u;   // image, hash rows, per-k-mer results of the tile
    p.wave_bytes = (p.wave_bytes + 15u) & ~15u;
    if (ix->rs > 128) {  // wide rows: no block histogram; the perfect search keeps a per-wave AND accumulator of rs words
        p.c_pad = 0;
        p.wave_bytes += 8u * ix->rs;
    }
    p.mod = ix->mod;
    p.unroll = (uint32_t)c->tune.search_unroll;
    if (cid::search_smem_bytes(p) > 160u * 1024u)
        return fail(CID_ERR_UNSUPPORTED, "LDS need %zu B exceeds 160 KiB (n_colors=%u k=%u n_hash=%u)",
                    cid::search_smem_bytes(p), ix->n_colors, ix->k, ix->n_hash);
    p.kmers = keys.ascii; p.codes = keys.codes; p.n_kmers = keys.n;
    p.tiles_per_block = pick_tiles_per_block(c, keys.n);
    return CID_OK;
}

// a caller's device pointers as keys of the index's k
cid::DevKeys caller_keys(const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_codes, const uint32_t *d_freq, size_t n_kmers) {
    return cid::DevKeys{d_kmers, d_codes, d_freq, n_kmers, ix ? ix->k : 0, nullptr};
}

// host results for k-mers that are already on the device
int search_count_to_host(cid_ctx *c, const cid_index *ix, const cid::DevKeys &keys, uint64_t *hits, uint64_t *n_unique, uint64_t *sum_unique_freq,
                         uint32_t *unique_colour) {
    const size_t C = ix->n_colors;
    void *d_out, *d_uc = nullptr;
    int rc = slot_reserve(c, S_OUT, 3 * C * 8, &d_out);
    if (rc) return rc;
    if (unique_colour) { rc = slot_reserve(c, S_UC, keys.n * 4, &d_uc); if (rc) return rc; }
    uint64_t *o = (uint64_t *)d_out;
    rc = cid::search_count_launch(c, ix, keys, o, n_unique ? o + C : nullptr, sum_unique_freq ? o + 2 * C : nullptr, (uint32_t *)d_uc);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(hits, o, C * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_unique) HIP_TRY(hipMemcpyAsync(n_unique, o + C, C * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_unique_freq) HIP_TRY(hipMemcpyAsync(sum_unique_freq, o + 2 * C, C * 8, hipMemcpyDeviceToHost, c->stream));
    if (unique_colour) HIP_TRY(hipMemcpyAsync(unique_colour, d_uc, keys.n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

// u64 words of the padded row -> the BitVec's w32 u32 words
void unpack_and_words(const uint64_t *row, size_t w32, uint32_t *words_le) {
    for (size_t w = 0; w < w32; ++w) words_le[w] = (uint32_t)(row[w / 2] >> (32 * (w & 1)));
}

int search_perfect_to_host(cid_ctx *c, const cid_index *ix, const cid::DevKeys &keys, uint32_t *and_words_le, int *any_row_missing) {
    void *d_out;
    int rc = slot_reserve(c, S_MISC, (size_t)ix->rs * 8 + 16, &d_out);
    if (rc) return rc;
    uint64_t *d_and = (uint64_t *)d_out;
    int *d_missing = (int *)(d_and + ix->rs);
    rc = cid::search_perfect_launch(c, ix, keys, d_and, d_missing);
    if (rc) return rc;
    std::vector<uint64_t> h(ix->rs);
    int missing = 0;
    HIP_TRY(hipMemcpyAsync(h.data(), d_and, (size_t)ix->rs * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&missing, d_missing, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *any_row_missing = missing ? 1 : 0;
    if (missing) memset(and_words_le, 0, (size_t)ix->w32 * 4);
    else unpack_and_words(h.data(), ix->w32, and_words_le);
    return CID_OK;
}

int check_segments_index(const cid_ctx *c, const cid_index *ix) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = check_not_mini(ix))) return rc;
    if (ix->rs > 128)
        return fail(CID_ERR_UNSUPPORTED, "segmented search needs at most 8192 colours (index has %u): one cid_search_count per segment instead", ix->n_colors);
    return CID_OK;
}

// device-resident inputs and outputs, n_segs < 2^32; `zero`: clear the outputs first (else they are added to); asynchronous on the ctx stream
int search_segments_launch(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, size_t n_segs, uint64_t n_kmers,
                           uint32_t *d_hits, uint8_t *d_missing, bool zero) {
    if (!d_seg_off || !d_hits) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    cid::SegmentParams q;
    int rc = fill_search_params(c, ix, caller_keys(ix, d_kmers, nullptr, nullptr, n_kmers), q.s);
    if (rc) return rc;
    q.seg_off = d_seg_off; q.n_segs = n_segs; q.hits = d_hits; q.missing = d_missing;
    if (zero) {
        HIP_TRY(hipMemsetAsync(d_hits, 0, n_segs * (size_t)ix->n_colors * 4, c->stream));
        if (d_missing) HIP_TRY(hipMemsetAsync(d_missing, 0, n_segs, c->stream));
    }
    HIP_TRY(cid::launch_search_segments(q, c->stream));
    return CID_OK;
}

// The segmented perfect search on device-resident inputs and outputs, asynchronous on the ctx stream.  `preset`: set the words to all
// ones and the flags to 0 first (else they are ANDed into / OR-ed: the second launch over a row that a chunk boundary cut)
int perfect_segments_launch(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, size_t n_segs, uint64_t n_kmers,
                            uint64_t *d_words, uint8_t *d_missing, bool preset) {
    cid::PerfectSegmentParams q;
    int rc = fill_search_params(c, ix, caller_keys(ix, d_kmers, nullptr, nullptr, n_kmers), q.s);
    if (rc) return rc;
    q.s.c_pad = 0;   // no histogram: the k-mer image, the hash rows and the tile's segment numbers are all the LDS the kernel needs
    q.s.wave_bytes = (uint32_t)cid::perfect_segments_wave_bytes(ix->k, ix->n_hash);
    q.seg_off = d_seg_off; q.n_segs = n_segs; q.and_words = d_words; q.missing = d_missing;
    if (preset) {
        HIP_TRY(hipMemsetAsync(d_words, 0xFF, n_segs * (size_t)ix->rs * 8, c->stream));
        HIP_TRY(hipMemsetAsync(d_missing, 0, n_segs, c->stream));
    }
    HIP_TRY(cid::launch_perfect_segments(q, c->stream));
    return CID_OK;
}

// A host seg_off of n_segs + 1 entries by the rules of cid_segplan.hpp; `bound`: max_len and what it counts, for the refusal
int check_host_seg_off(const uint64_t *seg_off, size_t n_segs, uint64_t max_len, const char *bound) {
    const cid::OffFault f = cid::check_seg_off(seg_off, n_segs, max_len);
    if (f.rule == cid::OFF_FIRST_NONZERO) return fail(CID_ERR_INVALID, "seg_off[0] must be 0");
    if (f.rule == cid::OFF_DECREASES) return fail(CID_ERR_INVALID, "seg_off decreases at segment %zu", (size_t)f.at);
    if (f.rule == cid::OFF_TOO_LONG) return fail(CID_ERR_INVALID, "segment %zu has %s or more", (size_t)f.at, bound);
    return CID_OK;
}

// segments per slice of a host-pointer call whose device copy of the results takes seg_bytes a segment (cid_ctx_tune "dense_report_bytes")
size_t segments_per_slice(const cid_ctx *c, size_t seg_bytes, size_t n_segs) {
    return std::min(std::max<size_t>(c->tune.dense_report_bytes / seg_bytes, 1), n_segs);
}

// The host-pointer form of the segmented searches.  The device copy of the results holds a slice of per_slice segments; a slice's k-mers
// go up in chunks of upload_chunk_bytes, each with its own offsets: the slice's segments clipped to the chunk (cid::plan_slice), so a
// segment cut by a chunk boundary goes through two launches that combine into the same row.  Per slice, on the ctx stream: its rows
// (and flags, if any) are preset; the offsets go up; per chunk the k-mers go up and launch(d_kmers, d_off, n_loc, nk, seg) searches nk
// k-mers whose n_loc segments start at segment `seg` of the slice; finish(s0, s1, the device copy of seg_off[s0 .. s1]) ends the slice,
// reads back what it has to and synchronises the stream: the next slice rewrites the host offsets and reuses the k-mer and offset slots.
struct SlicePreset { void *rows; size_t row_bytes; int fill; void *flags; };   // the entry point's S_REPORT and S_NK slots
template <class Launch, class Finish>
int walk_segments(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint64_t *seg_off, size_t n_segs, size_t per_slice, SlicePreset pre,
                  Launch launch, Finish finish) {
    const size_t k = ix->k, n_kmers = seg_off[n_segs];
    size_t chunk = upload_chunk_kmers(c, k);
    if (chunk > n_kmers) chunk = n_kmers ? n_kmers : 1;
    void *d_k, *d_off;
    int rc = slot_reserve(c, S_KMERS, chunk * k, &d_k); if (rc) return rc;
    std::vector<uint64_t> loc;
    std::vector<cid::SegPiece> pieces;
    for (size_t s0 = 0; s0 < n_segs; s0 += per_slice) {
        const size_t s1 = std::min(n_segs, s0 + per_slice);
        cid::plan_slice(seg_off, s0, s1, chunk, loc, pieces);
        HIP_TRY(hipMemsetAsync(pre.rows, pre.fill, (s1 - s0) * pre.row_bytes, c->stream));
        if (pre.flags) HIP_TRY(hipMemsetAsync(pre.flags, 0, s1 - s0, c->stream));
        rc = slot_reserve(c, S_SEQOFF, loc.size() * 8, &d_off); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d_off, loc.data(), loc.size() * 8, hipMemcpyHostToDevice, c->stream));
        for (const cid::SegPiece &pc : pieces) {
            HIP_TRY(hipMemcpyAsync(d_k, kmers + pc.k0 * k, pc.nk * k, hipMemcpyHostToDevice, c->stream));
            if ((rc = launch((const uint8_t *)d_k, (const uint64_t *)d_off + pc.loc0, pc.n_loc, pc.nk, pc.seg0 - s0))) return rc;
        }
        if ((rc = finish(s0, s1, (const uint64_t *)d_off))) return rc;
    }
    return CID_OK;
}

// The coverage search's two launches, device-resident inputs and outputs, asynchronous on the ctx stream.  d_rows: one row of rs u64 per
// window; the host form gathers a slice chunk by chunk (d_kmers, d_flags and d_rows then start at the chunk's first window) and
// computes the statistics once over the whole slice.
int fill_cover_params(cid_ctx *c, const cid_index *ix, const cid::DevKeys &keys, cid::CoverParams &q) {
    int rc = fill_search_params(c, ix, keys, q.s);
    if (rc) return rc;
    q.s.c_pad = 0;   // no histogram: the k-mer image and the hash rows are all the LDS the gather needs
    q.s.wave_bytes = (cid::kmer_img_bytes(ix->k) + cid::kWave * ix->n_hash * 4u + 15u) & ~15u;
    return CID_OK;
}

int search_cover_rows_launch(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint8_t *d_flags, uint64_t n_kmers, uint64_t *d_rows) {
    return cid::cover_rows_launch(c, ix, caller_keys(ix, d_kmers, nullptr, nullptr, n_kmers), d_flags, d_rows);
}

int search_cover_stats_launch(cid_ctx *c, const cid_index *ix, const uint64_t *d_seg_off, const uint8_t *d_flags, size_t n_segs, uint64_t n_kmers,
                              const uint64_t *d_rows, cid_cover *d_out) {
    cid::CoverParams q{};
    int rc = fill_cover_params(c, ix, cid::DevKeys{}, q);
    if (rc) return rc;
    q.s.n_kmers = n_kmers;
    q.flags = d_flags; q.rows = const_cast<uint64_t *>(d_rows); q.seg_off = d_seg_off; q.n_segs = n_segs; q.out = reinterpret_cast<uint32_t *>(d_out);
    HIP_TRY(cid::launch_cover_stats(q, c->stream));
    return CID_OK;
}

// one wave per (segment, 64-colour word): the grid's limit
int check_cover_grid(const cid_index *ix, size_t n_segs) {
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    if ((uint64_t)n_segs * ix->w64 >= (1ull << 33)) return fail(CID_ERR_INVALID, "%zu segments x %u colour words: 2^33 or more", n_segs, ix->w64);
    return CID_OK;
}

}  // namespace

namespace cid {

int cover_rows_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, const uint8_t *d_flags, uint64_t *d_rows) {
    CoverParams q{};
    int rc = fill_cover_params(c, ix, keys, q);
    if (rc) return rc;
    q.flags = d_flags; q.rows = d_rows;
    HIP_TRY(launch_cover_rows(q, c->stream));
    return CID_OK;
}

int search_count_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *d_hits, uint64_t *d_n_unique, uint64_t *d_sum_unique_freq,
                        uint32_t *d_unique_colour, bool zero_counters) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = check_not_mini(ix))) return rc;
    if (!d_hits) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    SearchParams p;
    rc = fill_search_params(c, ix, keys, p);
    if (rc) return rc;
    p.freq = keys.counts;
    p.hits = d_hits; p.n_unique = d_n_unique; p.sum_unique_freq = d_sum_unique_freq; p.unique_colour = d_unique_colour;
    p.want_unique = (d_n_unique || d_sum_unique_freq || d_unique_colour) ? 1u : 0u;
#ifdef CID_TUNE_BUILD
    p.mixed = c->tune.search_mixed ? 1u : 0u;
    if (c->tune.search_persist && ix->rs <= 128 && keys.n >= (1u << 16)) {   // persistent grid, one work queue per XCD (cid_search.hip)
        void *d_q;
        rc = slot_reserve(c, S_QUEUE, 8 * 128, &d_q); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_q, 0, 8 * 128, c->stream));
        p.queues = (uint32_t *)d_q;
        p.persist_grid = c->n_cu * cid::search_count_blocks_per_cu(p);
        if (p.persist_grid <= 0) p.queues = nullptr;
    }
#endif
    const size_t cb = (size_t)ix->n_colors * 8;
    if (zero_counters) {
        HIP_TRY(hipMemsetAsync(d_hits, 0, cb, c->stream));
        if (d_n_unique) HIP_TRY(hipMemsetAsync(d_n_unique, 0, cb, c->stream));
        if (d_sum_unique_freq) HIP_TRY(hipMemsetAsync(d_sum_unique_freq, 0, cb, c->stream));
    }
    HIP_TRY(cid::launch_search_count(p, c->stream));
    return CID_OK;
}

// Host-pointer form.  The batch goes through in chunks: the H2D copy of chunk i+1 (copy stream) runs beside the kernel of chunk i
// (ctx stream), and the per-k-mer results of chunk i-1 come back while both run; counters accumulate on the device over the
// chunks.  What is left is the PCIe time of 31+4 bytes in and 4 bytes out per k-mer.
// Host k-mers in, per-k-mer results out to the host, the 3*C counters (hits | n_unique | sum_unique_freq) left on the device in
// *d_counters (the ctx's S_OUT slot); returns with both streams drained
int search_count_host_input(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint32_t *freq, size_t n_kmers, bool want_unique,
                            uint32_t *unique_colour, uint64_t **d_counters) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (n_kmers && !kmers) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t C = ix->n_colors, k = ix->k;
    size_t chunk = upload_chunk_kmers(c, k);
    if (chunk >= n_kmers || c->stream != c->own_stream) chunk = n_kmers ? n_kmers : 1;   // a borrowed stream: keep everything on it
    void *d_k, *d_f = nullptr, *d_out, *d_uc = nullptr;
    const size_t two = chunk < n_kmers ? 2 : 1;
    rc = slot_reserve(c, S_KMERS, two * chunk * k, &d_k); if (rc) return rc;
    if (freq) { rc = slot_reserve(c, S_FREQ, two * chunk * 4, &d_f); if (rc) return rc; }
    rc = slot_reserve(c, S_OUT, 3 * C * 8, &d_out); if (rc) return rc;
    if (unique_colour) { rc = slot_reserve(c, S_UC, two * chunk * 4, &d_uc); if (rc) return rc; }
    uint64_t *o = (uint64_t *)d_out;
    HIP_TRY(hipMemsetAsync(o, 0, 3 * C * 8, c->stream));
    const bool piped = two == 2;
    hipStream_t cs = piped ? c->copy_stream : c->stream;
    size_t prev_first = 0, prev_n = 0;
    int prev_b = 0;
    size_t i = 0;
    for (size_t first = 0; first < n_kmers || first == 0; first += chunk, ++i) {
        const size_t nk = n_kmers - first < chunk ? n_kmers - first : chunk;
        const int b = (int)(i & 1);
        uint8_t *dk = (uint8_t *)d_k + (size_t)b * chunk * k;
        uint32_t *df = d_f ? (uint32_t *)d_f + (size_t)b * chunk : nullptr;
        uint32_t *du = d_uc ? (uint32_t *)d_uc + (size_t)b * chunk : nullptr;
        if (piped && i >= 2) HIP_TRY(hipStreamWaitEvent(cs, c->ev_done[b], 0));     // buffer b's previous kernel has consumed it
        if (nk) HIP_TRY(hipMemcpyAsync(dk, kmers + first * k, nk * k, hipMemcpyHostToDevice, cs));
        if (nk && freq) HIP_TRY(hipMemcpyAsync(df, freq + first, nk * 4, hipMemcpyHostToDevice, cs));
        if (piped) {
            HIP_TRY(hipEventRecord(c->ev_copied[b], cs));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
        }
        rc = search_count_launch(c, ix, DevKeys{dk, nullptr, df, nk, ix->k, c}, o, want_unique ? o + C : nullptr, want_unique ? o + 2 * C : nullptr, du, false);
        if (rc) return rc;
        if (piped) HIP_TRY(hipEventRecord(c->ev_done[b], c->stream));
        // the previous chunk's per-k-mer results: its kernel finished while this chunk was copied in
        if (unique_colour && prev_n) {
            if (piped) HIP_TRY(hipStreamWaitEvent(cs, c->ev_done[prev_b], 0));
            HIP_TRY(hipMemcpyAsync(unique_colour + prev_first, (uint32_t *)d_uc + (size_t)prev_b * chunk, prev_n * 4, hipMemcpyDeviceToHost, cs));
        }
        prev_first = first; prev_n = nk; prev_b = b;
        if (n_kmers == 0) break;
    }
    if (unique_colour && prev_n)
        HIP_TRY(hipMemcpyAsync(unique_colour + prev_first, (uint32_t *)d_uc + (size_t)prev_b * chunk, prev_n * 4, hipMemcpyDeviceToHost, c->stream));
    if (piped) HIP_TRY(hipStreamSynchronize(cs));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *d_counters = o;
    return CID_OK;
}

// ------------------------------------------------------------------------------------------------ a4

int search_perfect_launch(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *d_and, int *d_missing) {
    int rc = check_not_mini(ix);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_and, 0xFF, (size_t)ix->rs * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_missing, 0, 16, c->stream));
    SearchParams p;
    rc = fill_search_params(c, ix, keys, p);
    if (rc) return rc;
    p.and_words = d_and; p.missing = d_missing;
    HIP_TRY(launch_search_perfect(p, c->stream));
    return CID_OK;
}

int search_count_keys(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint64_t *hits, uint64_t *n_unique, uint64_t *sum_unique_freq,
                      uint32_t *unique_colour) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (!hits) return fail(CID_ERR_INVALID, "null argument");
    if (ix->k != keys.k) return fail(CID_ERR_INVALID, "k-mer set k=%u, index k=%u", keys.k, ix->k);
    HIP_TRY(hipSetDevice(c->device));
    return search_count_to_host(c, ix, keys, hits, n_unique, sum_unique_freq, unique_colour);
}

int search_perfect_keys(cid_ctx *c, const cid_index *ix, const DevKeys &keys, uint32_t *and_words_le, int *any_row_missing) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (!and_words_le || !any_row_missing) return fail(CID_ERR_INVALID, "null argument");
    if (keys.n == 0) return fail(CID_ERR_INVALID, "perfect search needs at least one k-mer (src/perfect_search.rs:22-23)");
    if (ix->k != keys.k) return fail(CID_ERR_INVALID, "k-mer set k=%u, index k=%u", keys.k, ix->k);
    HIP_TRY(hipSetDevice(c->device));
    return search_perfect_to_host(c, ix, keys, and_words_le, any_row_missing);
}

}  // namespace cid

extern "C" {

int cid_search_count_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint32_t *d_freq, size_t n_kmers,
                         uint64_t *d_hits, uint64_t *d_n_unique, uint64_t *d_sum_unique_freq, uint32_t *d_unique_colour) {
    return cid::search_count_launch(c, ix, caller_keys(ix, d_kmers, nullptr, d_freq, n_kmers), d_hits, d_n_unique, d_sum_unique_freq, d_unique_colour);
}

int cid_search_count_codes_dev(cid_ctx *c, const cid_index *ix, const uint64_t *d_codes, const uint32_t *d_freq, size_t n_kmers,
                               uint64_t *d_hits, uint64_t *d_n_unique, uint64_t *d_sum_unique_freq, uint32_t *d_unique_colour) {
    return cid::search_count_launch(c, ix, caller_keys(ix, nullptr, d_codes, d_freq, n_kmers), d_hits, d_n_unique, d_sum_unique_freq, d_unique_colour);
}

// One colour stripe of a wider index: per-colour hits are final; per-k-mer popcounts and unique
// candidates accumulate across the stripes' calls and are resolved by cid_search_unique_finalize_dev.
int cid_search_count_stripe_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_codes, size_t n_kmers,
                                uint32_t colour_base, uint64_t *d_hits, uint32_t *d_fact) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = check_not_mini(ix))) return rc;
    if (!d_hits || !d_fact) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    cid::SearchParams p;
    rc = fill_search_params(c, ix, caller_keys(ix, d_kmers, d_codes, nullptr, n_kmers), p);
    if (rc) return rc;
    p.hits = d_hits; p.colour_base = colour_base; p.fact = d_fact;
    HIP_TRY(hipMemsetAsync(d_hits, 0, (size_t)ix->n_colors * 8, c->stream));
    HIP_TRY(cid::launch_search_count(p, c->stream));
    return CID_OK;
}

int cid_search_unique_finalize_dev(cid_ctx *c, const uint32_t *d_fact, const uint32_t *d_freq,
                                   size_t n_kmers, uint32_t n_colors_total, uint64_t *d_n_unique, uint64_t *d_sum_unique_freq,
                                   uint32_t *d_unique_colour) {
    if (!c || (n_kmers && !d_fact) || n_colors_total == 0 || n_colors_total > (1u << 20)) return fail(CID_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(cid::launch_unique_finalize(d_fact, d_freq, n_kmers, n_colors_total, d_n_unique, d_sum_unique_freq,
                                        d_unique_colour, c->stream));
    return CID_OK;
}

// Perfect search on one stripe: the stripe's AND words are final; d_zero_acc[n_kmers] (preset to all-ones) collects,
// per k-mer, the seeds whose row is all-zero in every stripe so far — any bit left at the end means "row absent".
int cid_search_perfect_stripe_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_codes, size_t n_kmers,
                                  uint64_t *d_and_words, uint32_t *d_zero_acc) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = check_not_mini(ix))) return rc;
    if (!d_and_words || !d_zero_acc) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    void *d_scratch;
    rc = slot_reserve(c, S_MISC, 16, &d_scratch);
    if (rc) return rc;
    cid::SearchParams p;
    rc = fill_search_params(c, ix, caller_keys(ix, d_kmers, d_codes, nullptr, n_kmers), p);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_and_words, 0xFF, (size_t)ix->rs * 8, c->stream));
    p.and_words = d_and_words; p.missing = (int *)d_scratch; p.zero_acc = d_zero_acc;
    HIP_TRY(cid::launch_search_perfect(p, c->stream));
    return CID_OK;
}

int cid_search_count(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint32_t *freq, size_t n_kmers,
                     uint64_t *hits, uint64_t *n_unique, uint64_t *sum_unique_freq, uint32_t *unique_colour) {
    if (!hits) return fail(CID_ERR_INVALID, "null argument");
    uint64_t *o = nullptr;
    int rc = cid::search_count_host_input(c, ix, kmers, freq, n_kmers, n_unique || sum_unique_freq || unique_colour, unique_colour, &o);
    if (rc) return rc;
    const size_t C = ix->n_colors;
    HIP_TRY(hipMemcpyAsync(hits, o, C * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_unique) HIP_TRY(hipMemcpyAsync(n_unique, o + C, C * 8, hipMemcpyDeviceToHost, c->stream));
    if (sum_unique_freq) HIP_TRY(hipMemcpyAsync(sum_unique_freq, o + 2 * C, C * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

int cid_search_perfect(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, size_t n_kmers, uint32_t *and_words_le,
                       int *any_row_missing) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (!and_words_le || !any_row_missing || (n_kmers && !kmers)) return fail(CID_ERR_INVALID, "null argument");
    if (n_kmers == 0) return fail(CID_ERR_INVALID, "perfect search needs at least one k-mer (src/perfect_search.rs:22-23)");
    HIP_TRY(hipSetDevice(c->device));
    void *d_k;
    rc = slot_reserve(c, S_KMERS, n_kmers * ix->k, &d_k);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_k, kmers, n_kmers * ix->k, hipMemcpyHostToDevice, c->stream));
    return search_perfect_to_host(c, ix, cid::DevKeys{(const uint8_t *)d_k, nullptr, nullptr, n_kmers, ix->k, c}, and_words_le, any_row_missing);
}

// ------------------------------------------------------------------------------------------------ segmented search (cid_segments.hip)

int cid_search_segments_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, size_t n_segs, uint64_t n_kmers,
                            uint32_t *d_hits, uint8_t *d_any_row_missing) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    return search_segments_launch(c, ix, d_kmers, d_seg_off, n_segs, n_kmers, d_hits, d_any_row_missing, true);
}

// Host-pointer form (walk_segments): a slice's counters are zeroed, every chunk's launch adds into them, and they come back per slice.
int cid_search_segments(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint64_t *seg_off, size_t n_segs, uint32_t *hits,
                        uint8_t *any_row_missing) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (!seg_off || !hits) return fail(CID_ERR_INVALID, "null argument");
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    if ((rc = check_host_seg_off(seg_off, n_segs, 1ull << 32, "2^32 k-mers"))) return rc;
    if (seg_off[n_segs] && !kmers) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t C = ix->n_colors, per_slice = segments_per_slice(c, C * 4, n_segs);
    void *d_hits, *d_miss;
    rc = slot_reserve(c, S_REPORT, per_slice * C * 4, &d_hits); if (rc) return rc;
    rc = slot_reserve(c, S_NK, per_slice, &d_miss); if (rc) return rc;
    return walk_segments(c, ix, kmers, seg_off, n_segs, per_slice, SlicePreset{d_hits, C * 4, 0, d_miss},
        [&](const uint8_t *d_k, const uint64_t *d_off, size_t n_loc, size_t nk, size_t seg) {
            return search_segments_launch(c, ix, d_k, d_off, n_loc, nk, (uint32_t *)d_hits + seg * C, (uint8_t *)d_miss + seg, false); },
        [&](size_t s0, size_t s1, const uint64_t *) -> int {
            HIP_TRY(hipMemcpyAsync(hits + s0 * C, d_hits, (s1 - s0) * C * 4, hipMemcpyDeviceToHost, c->stream));
            if (any_row_missing) HIP_TRY(hipMemcpyAsync(any_row_missing + s0, d_miss, s1 - s0, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return CID_OK;
        });
}

// ------------------------------------------------------------------------------------------------ segmented perfect search (cid_perfect_segments.hip)

int cid_search_perfect_segments_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, size_t n_segs,
                                    uint64_t n_kmers, uint64_t *d_and_words, uint8_t *d_any_row_missing) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    if (!d_seg_off || !d_and_words || (n_kmers && !d_kmers)) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (!d_any_row_missing) {   // the words of a flagged segment are zero whether or not the caller wants the flags
        void *d_miss;
        rc = slot_reserve(c, S_NK, n_segs, &d_miss); if (rc) return rc;
        d_any_row_missing = (uint8_t *)d_miss;
    }
    rc = perfect_segments_launch(c, ix, d_kmers, d_seg_off, n_segs, n_kmers, d_and_words, d_any_row_missing, true);
    if (rc) return rc;
    HIP_TRY(cid::launch_perfect_segments_finish(d_and_words, d_any_row_missing, d_seg_off, n_segs, ix->rs, ix->n_colors, c->stream));
    return CID_OK;
}

// Host-pointer form (walk_segments): a slice's words are preset to all ones and its flags to 0 once, every chunk's launch ANDs and ORs into
// them, and the finish kernel runs once per slice, over the slice's true offsets.
int cid_search_perfect_segments(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint64_t *seg_off, size_t n_segs,
                                uint32_t *and_words_le, uint8_t *any_row_missing) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (!seg_off || !and_words_le) return fail(CID_ERR_INVALID, "null argument");
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    if ((rc = check_host_seg_off(seg_off, n_segs, 1ull << 32, "2^32 k-mers"))) return rc;
    if (seg_off[n_segs] && !kmers) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t rs = ix->rs, w32 = ix->w32, per_slice = segments_per_slice(c, rs * 8, n_segs);
    void *d_words, *d_miss;
    rc = slot_reserve(c, S_REPORT, per_slice * rs * 8, &d_words); if (rc) return rc;
    rc = slot_reserve(c, S_NK, per_slice, &d_miss); if (rc) return rc;
    std::vector<uint64_t> h_words;
    return walk_segments(c, ix, kmers, seg_off, n_segs, per_slice, SlicePreset{d_words, rs * 8, 0xFF, d_miss},
        [&](const uint8_t *d_k, const uint64_t *d_off, size_t n_loc, size_t nk, size_t seg) {
            return perfect_segments_launch(c, ix, d_k, d_off, n_loc, nk, (uint64_t *)d_words + seg * rs, (uint8_t *)d_miss + seg, false); },
        [&](size_t s0, size_t s1, const uint64_t *d_true_off) -> int {
            const size_t ns = s1 - s0;
            HIP_TRY(cid::launch_perfect_segments_finish((uint64_t *)d_words, (const uint8_t *)d_miss, d_true_off, ns, (uint32_t)rs, ix->n_colors, c->stream));
            h_words.resize(ns * rs);
            HIP_TRY(hipMemcpyAsync(h_words.data(), d_words, ns * rs * 8, hipMemcpyDeviceToHost, c->stream));
            if (any_row_missing) HIP_TRY(hipMemcpyAsync(any_row_missing + s0, d_miss, ns, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (size_t s = 0; s < ns; ++s) unpack_and_words(&h_words[s * rs], w32, and_words_le + (s0 + s) * w32);
            return CID_OK;
        });
}

// ------------------------------------------------------------------------------------------------ nearest segment per group (cid_nearest.hip)

int cid_search_nearest_segments_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, size_t n_segs,
                                    uint64_t n_kmers, const uint64_t *d_group_off, size_t n_groups, cid_nearest *d_out) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_groups == 0 || n_segs == 0) return CID_OK;
    if (n_segs >= (1ull << 32) || n_groups >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or groups, or more");
    if (!d_seg_off || !d_group_off || !d_out || (n_kmers && !d_kmers)) return fail(CID_ERR_INVALID, "null argument");
    if (!aligned16(d_out)) return fail(CID_ERR_INVALID, "d_out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    void *d_hits;
    rc = slot_reserve(c, S_REPORT, n_segs * (size_t)ix->n_colors * 4, &d_hits); if (rc) return rc;
    rc = search_segments_launch(c, ix, d_kmers, d_seg_off, n_segs, n_kmers, (uint32_t *)d_hits, nullptr, true); if (rc) return rc;
    HIP_TRY(cid::launch_nearest_preset(d_out, (uint64_t)n_groups * ix->n_colors, c->stream));
    cid::NearestParams q{(const uint32_t *)d_hits, d_seg_off, d_group_off, n_groups, 0, 0, n_segs, ix->n_colors, reinterpret_cast<uint4 *>(d_out)};
    HIP_TRY(cid::launch_nearest_groups(q, c->stream));
    return CID_OK;
}

// Host-pointer form (walk_segments).  The cells of all groups stay on the device for the whole call, preset once; a slice's counters are
// cid_search_segments', and one k_nearest_groups launch ends the slice and merges its part of every group it touches into the group's cells.
// A cut may fall inside a group: the earlier slice holds the lower segment numbers, and the order is total, so the result is that of one pass.
int cid_search_nearest_segments(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint64_t *seg_off, size_t n_segs,
                                const uint64_t *group_off, size_t n_groups, cid_nearest *out) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_groups == 0 || n_segs == 0) return CID_OK;
    if (!seg_off || !group_off || !out) return fail(CID_ERR_INVALID, "null argument");
    if (n_segs >= (1ull << 32) || n_groups >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or groups, or more");
    if ((rc = check_host_seg_off(seg_off, n_segs, 1ull << 32, "2^32 k-mers"))) return rc;
    const cid::OffFault g = cid::check_group_off(group_off, n_groups, n_segs);
    if (g.rule == cid::OFF_FIRST_NONZERO) return fail(CID_ERR_INVALID, "group_off[0] must be 0");
    if (g.rule == cid::OFF_DECREASES) return fail(CID_ERR_INVALID, "group_off decreases at group %zu", (size_t)g.at);
    if (g.rule == cid::OFF_WRONG_END) return fail(CID_ERR_INVALID, "group_off ends at %llu, not at the %zu segments", (unsigned long long)g.at, n_segs);
    if (seg_off[n_segs] && !kmers) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t C = ix->n_colors, per_slice = segments_per_slice(c, C * 4, n_segs);
    void *d_hits, *d_groups, *d_cells;
    rc = slot_reserve(c, S_REPORT, per_slice * C * 4, &d_hits); if (rc) return rc;
    rc = slot_reserve(c, S_ROWIDS, (n_groups + 1) * 8, &d_groups); if (rc) return rc;
    rc = slot_reserve(c, S_WORDS, n_groups * C * sizeof(cid_nearest), &d_cells); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_groups, group_off, (n_groups + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cid::launch_nearest_preset(d_cells, (uint64_t)n_groups * C, c->stream));
    size_t ga = 0;               // the first group that reaches into the slice
    rc = walk_segments(c, ix, kmers, seg_off, n_segs, per_slice, SlicePreset{d_hits, C * 4, 0, nullptr},
        [&](const uint8_t *d_k, const uint64_t *d_off, size_t n_loc, size_t nk, size_t seg) {
            return search_segments_launch(c, ix, d_k, d_off, n_loc, nk, (uint32_t *)d_hits + seg * C, nullptr, false); },
        [&](size_t s0, size_t s1, const uint64_t *d_true_off) -> int {
            while (group_off[ga + 1] <= s0) ++ga;            // (group_off ends at n_segs > s0)
            size_t gb = ga;                                  // the last group that starts before the slice's end
            while (gb + 1 < n_groups && group_off[gb + 1] < s1) ++gb;
            cid::NearestParams q{(const uint32_t *)d_hits, d_true_off, (const uint64_t *)d_groups + ga, gb - ga + 1, ga, s0, s1, (uint32_t)C,
                                 reinterpret_cast<uint4 *>(d_cells)};
            HIP_TRY(cid::launch_nearest_groups(q, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return CID_OK;
        });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_cells, n_groups * C * sizeof(cid_nearest), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

// ------------------------------------------------------------------------------------------------ coverage search (cid_cover.hip)

int cid_search_cover_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_kmers, const uint64_t *d_seg_off, const uint8_t *d_flags, size_t n_segs,
                         uint64_t n_kmers, cid_cover *d_out) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (!d_seg_off || !d_out || (n_kmers && !d_kmers)) return fail(CID_ERR_INVALID, "null argument");
    if (!aligned16(d_out)) return fail(CID_ERR_INVALID, "d_out must be 16-byte aligned");
    if ((rc = check_cover_grid(ix, n_segs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    void *d_rows;
    rc = slot_reserve(c, S_WORDS, (size_t)n_kmers * ix->rs * 8, &d_rows); if (rc) return rc;
    rc = search_cover_rows_launch(c, ix, d_kmers, d_flags, n_kmers, (uint64_t *)d_rows); if (rc) return rc;
    return search_cover_stats_launch(c, ix, d_seg_off, d_flags, n_segs, n_kmers, (const uint64_t *)d_rows, d_out);
}

// Host-pointer form.  The call is cut at whole segments into slices whose device scratch (8 * rs bytes per window) plus output (32 bytes per
// segment and colour) fit dense_report_bytes: a segment's windows are never split, so the run statistics need no stitching.  A slice's
// k-mers go up in chunks of upload_chunk_bytes, one k_cover_rows launch per chunk (chunks start on a tile boundary); its flags and offsets
// go up whole, and one k_cover_stats launch ends the slice.
int cid_search_cover(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint64_t *seg_off, const uint8_t *flags, size_t n_segs,
                     cid_cover *out) {
    int rc = check_segments_index(c, ix);
    if (rc) return rc;
    if (n_segs == 0) return CID_OK;
    if (!seg_off || !out) return fail(CID_ERR_INVALID, "null argument");
    if (n_segs >= (1ull << 32)) return fail(CID_ERR_INVALID, "2^32 segments or more");
    if ((rc = check_host_seg_off(seg_off, n_segs, (1ull << 32) - 128, "2^32 - 128 windows"))) return rc;
    if (seg_off[n_segs] && !kmers) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t C = ix->n_colors, k = ix->k, row_bytes = (size_t)ix->rs * 8, cell_bytes = C * sizeof(cid_cover);
    const unsigned long long budget = c->tune.dense_report_bytes;
    const size_t chunk = upload_chunk_kmers(c, k);
    std::vector<uint64_t> loc;
    for (size_t s0 = 0; s0 < n_segs;) {
        size_t s1 = s0;
        while (s1 < n_segs && (seg_off[s1 + 1] - seg_off[s0]) * row_bytes + (s1 + 1 - s0) * cell_bytes <= budget) ++s1;
        if (s1 == s0)
            return fail(CID_ERR_UNSUPPORTED, "segment %zu (%llu windows, %zu colours) needs %llu bytes of device scratch and output: more than dense_report_bytes = %llu",
                        s0, (unsigned long long)(seg_off[s0 + 1] - seg_off[s0]), C,
                        (unsigned long long)((seg_off[s0 + 1] - seg_off[s0]) * row_bytes + cell_bytes), budget);
        if ((rc = check_cover_grid(ix, s1 - s0))) return rc;
        const uint64_t w_first = seg_off[s0], n_win = seg_off[s1] - w_first;
        loc.resize(s1 - s0 + 1);
        for (size_t s = s0; s <= s1; ++s) loc[s - s0] = seg_off[s] - w_first;
        void *d_k = nullptr, *d_rows = nullptr, *d_fl = nullptr, *d_off, *d_out;
        rc = slot_reserve(c, S_SEQOFF, loc.size() * 8, &d_off); if (rc) return rc;
        rc = slot_reserve(c, S_REPORT, (s1 - s0) * cell_bytes, &d_out); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d_off, loc.data(), loc.size() * 8, hipMemcpyHostToDevice, c->stream));
        if (n_win) {
            rc = slot_reserve(c, S_KMERS, std::min<uint64_t>(chunk, n_win) * k, &d_k); if (rc) return rc;
            rc = slot_reserve(c, S_WORDS, n_win * row_bytes, &d_rows); if (rc) return rc;
            if (flags) {
                rc = slot_reserve(c, S_NK, n_win, &d_fl); if (rc) return rc;
                HIP_TRY(hipMemcpyAsync(d_fl, flags + w_first, n_win, hipMemcpyHostToDevice, c->stream));
            }
        }
        for (uint64_t w0 = 0; w0 < n_win; w0 += chunk) {
            const uint64_t nw = std::min<uint64_t>(chunk, n_win - w0);
            HIP_TRY(hipMemcpyAsync(d_k, kmers + (w_first + w0) * k, nw * k, hipMemcpyHostToDevice, c->stream));
            rc = search_cover_rows_launch(c, ix, (const uint8_t *)d_k, d_fl ? (const uint8_t *)d_fl + w0 : nullptr, nw, (uint64_t *)d_rows + w0 * ix->rs);
            if (rc) return rc;
        }
        rc = search_cover_stats_launch(c, ix, (const uint64_t *)d_off, (const uint8_t *)d_fl, s1 - s0, n_win, (const uint64_t *)d_rows, (cid_cover *)d_out);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(out + s0 * C, d_out, (s1 - s0) * cell_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        s0 = s1;
    }
    return CID_OK;
}

}  // extern C
