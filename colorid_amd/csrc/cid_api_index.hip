// C ABI of libcolorid_hip.so, part 2: the device-resident index — BigsyMapNew.map (src/bigsi.rs:19-27) as a dense bit matrix:
// create / fill from .bxi rows and records / read back / Bloom inserts (src/simple_bloom.rs:19-26).  Kernels: cid_index.hip.
#include "cid_api_common.hpp"

using cid::aligned16;
using cid::fail;
using cid::pick_tiles_per_block;
using cid::slot_reserve;
using cid::stage_records;
using namespace cid::slots;

namespace cid {
uint32_t index_k(const cid_index *ix) { return ix->k; }
uint32_t index_rs(const cid_index *ix) { return ix->rs; }
ModMagic index_mod(const cid_index *ix) { return ix->mod; }
uint32_t index_n_colors(const cid_index *ix) { return ix->n_colors; }
uint32_t index_n_hash(const cid_index *ix) { return ix->n_hash; }
uint32_t index_m_size(const cid_index *ix) { return ix->m_size; }
const uint64_t *index_matrix(const cid_index *ix) { return ix->mat; }

int check_ready(const cid_ctx *c, const cid_index *ix) {
    if (!c || !ix) return fail(CID_ERR_INVALID, "null ctx/index");
    if (!ix->finalized) return fail(CID_ERR_STATE, "index not finalized");
    if (ix->ctx->device != c->device) return fail(CID_ERR_INVALID, "index lives on device %d, ctx on %d", ix->ctx->device, c->device);
    return CID_OK;
}
int check_batch(const HostOffsets &h, uint32_t stride_d, const void *bases) {
    if (!h.seq_off || !h.read_seq0) return fail(CID_ERR_INVALID, "null argument");
    if (stride_d == 0) return fail(CID_ERR_INVALID, "stride_d must be >= 1");
    if (h.n_reads == 0) return CID_OK;
    if (h.read_seq0[h.n_reads] > h.n_seqs) return fail(CID_ERR_INVALID, "read_seq0 points past n_seqs");
    if (h.seq_off[h.n_seqs] && !bases) return fail(CID_ERR_INVALID, "null bases");
    return CID_OK;
}
int batch_fail(const BatchFault &f) {
    static const char *const what[] = {"", "read_seq0 not monotonic at read", "read_seq0 points past n_seqs at read", "seq_off not monotonic at seq"};
    return f.rule ? fail(CID_ERR_INVALID, "%s %llu", what[f.rule], (unsigned long long)f.at) : CID_OK;
}
// `search` is not defined on minimizer indices ("An index with minimizers (.mxi) is used, but not available for this
// function", src/main.rs:569-573)
int check_not_mini(const cid_index *ix) {
    return ix->m_size ? fail(CID_ERR_UNSUPPORTED, "search on a minimizer (.mxi) index is not defined by the reference") : CID_OK;
}
// a Bloom insert of n_kmers k-mers into ix; the caller names the k-mers (kmers or codes) and their colour (colour or colour_of_kmer)
static InsertParams insert_params(const cid_index *ix, size_t n_kmers) {
    InsertParams p{};
    p.mat = ix->mat; p.rs = ix->rs; p.n_hash = ix->n_hash; p.k = ix->k; p.n_colors = ix->n_colors;
    p.tiles_per_block = pick_tiles_per_block(ix->ctx, n_kmers);
    p.m_size = ix->m_size; p.mod = ix->mod; p.n_kmers = n_kmers;
    return p;
}
}  // namespace cid

extern "C" {

int cid_index_create(cid_ctx *c, uint64_t bloom_size, uint32_t num_hash, uint32_t k_size, uint32_t n_colors,
                     int hash_variant, cid_index **out) {
    if (!c || !out) return fail(CID_ERR_INVALID, "null ctx/out");
    *out = nullptr;
    if (hash_variant < 0 || hash_variant >= CID_HASH_VARIANTS) return fail(CID_ERR_UNSUPPORTED, "hash variant %d", hash_variant);
    if (bloom_size == 0 || num_hash == 0 || n_colors == 0 || k_size == 0) return fail(CID_ERR_INVALID, "zero parameter");
    if (k_size > cid::kMaxK) return fail(CID_ERR_UNSUPPORTED, "k_size %u > %u", k_size, cid::kMaxK);
    if (num_hash > 32) return fail(CID_ERR_UNSUPPORTED, "num_hash %u > 32", num_hash);
    if (bloom_size > (1ull << 32)) return fail(CID_ERR_UNSUPPORTED, "bloom_size %llu > 2^32", (unsigned long long)bloom_size);
    if (n_colors > (1u << 20)) return fail(CID_ERR_UNSUPPORTED, "n_colors %u > 2^20", n_colors);
    cid_index *ix = new (std::nothrow) cid_index();
    if (!ix) return fail(CID_ERR_NOMEM, "index");
    ix->ctx = c;
    ix->m = bloom_size; ix->n_hash = num_hash; ix->k = k_size; ix->n_colors = n_colors;
    ix->w32 = (n_colors + 31) / 32;
    ix->w64 = (n_colors + 63) / 64;
    ix->rs = cid::row_stride_words(n_colors);
    const cid::ModMagicHost mh = cid::make_mod_magic(bloom_size);
    ix->mod = cid::ModMagic{mh.m, mh.magic, mh.shift, mh.flags | ((uint32_t)hash_variant << 8),
                            hash_variant == CID_HASH_XXH3_V07 ? 0x165667B19E3779F9ULL : 0x165667919E3779F9ULL};
    hipError_t e = hipSetDevice(c->device);
    const size_t bytes = (size_t)bloom_size * ix->rs * 8;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&ix->mat), bytes);
    if (e != hipSuccess) { delete ix; return fail(CID_ERR_NOMEM, "hipMalloc(%zu) for the index: %s", bytes, hipGetErrorString(e)); }
    e = hipMemsetAsync(ix->mat, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(ix->mat); delete ix; return fail(CID_ERR_HIP, "memset: %s", hipGetErrorString(e)); }
    *out = ix;
    return CID_OK;
}

int cid_index_set_minimizer(cid_index *ix, uint32_t m_size) {
    if (!ix) return fail(CID_ERR_INVALID, "null index");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (m_size == 0 || m_size > ix->k) return fail(CID_ERR_INVALID, "minimizer size %u must be in 1..k_size (%u)", m_size, ix->k);
    ix->m_size = m_size;
    return CID_OK;
}

int cid_index_set_hash_variant(cid_index *ix, int hash_variant) {
    if (!ix) return fail(CID_ERR_INVALID, "null index");
    if (hash_variant < 0 || hash_variant >= CID_HASH_VARIANTS) return fail(CID_ERR_UNSUPPORTED, "hash variant %d", hash_variant);
    HIP_TRY(hipSetDevice(ix->ctx->device));
    HIP_TRY(hipStreamSynchronize(ix->ctx->stream));
    ix->mod.flags = (ix->mod.flags & 0xFFu) | ((uint32_t)hash_variant << 8);
    ix->mod.xmul = hash_variant == CID_HASH_XXH3_V07 ? 0x165667B19E3779F9ULL : 0x165667919E3779F9ULL;
    return CID_OK;
}

int cid_index_put_rows(cid_index *ix, const uint64_t *row_ids, const uint32_t *words_le, size_t n_rows) {
    if (!ix || (n_rows && (!row_ids || !words_le))) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t tail_mask = cid::tail_mask(ix->n_colors);
    for (size_t i = 0; i < n_rows; ++i) {
        if (row_ids[i] >= ix->m) return fail(CID_ERR_INVALID, "row id %llu >= bloom_size", (unsigned long long)row_ids[i]);
        if (words_le[i * ix->w32 + ix->w32 - 1] & ~tail_mask) return fail(CID_ERR_INVALID, "row %llu has bits beyond n_colors", (unsigned long long)row_ids[i]);
    }
    const size_t batch = 1u << 22;
    for (size_t r0 = 0; r0 < n_rows; r0 += batch) {
        const size_t nr = n_rows - r0 < batch ? n_rows - r0 : batch;
        void *d_ids, *d_words;
        int rc = slot_reserve(c, S_ROWIDS, nr * 8, &d_ids);
        if (rc) return rc;
        rc = slot_reserve(c, S_WORDS, nr * ix->w32 * 4, &d_words);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(d_ids, row_ids + r0, nr * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_words, words_le + r0 * ix->w32, nr * ix->w32 * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(cid::launch_put_rows(ix->mat, ix->rs, (const uint64_t *)d_ids, (const uint32_t *)d_words, ix->w32, nr, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CID_OK;
}

}  // extern "C"

// records of a file with n_colors_total colours; the index takes the colours [colour_base, colour_base + ix->n_colors) (colour_base a
// multiple of 32: whole u32 words)
int cid::index_put_records_slice(cid_index *ix, const uint8_t *records, size_t n_records, uint32_t n_colors_total, uint32_t colour_base) {
    if (!ix || (n_records && !records)) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (colour_base % 32u || (uint64_t)colour_base + ix->n_colors > n_colors_total) return fail(CID_ERR_INVALID, "stripe [%u, +%u) of %u colours",
        colour_base, ix->n_colors, n_colors_total);
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t w32_rec = (n_colors_total + 31u) / 32u;
    return stage_records(c, records, n_records, w32_rec, ix->w32, [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
        return cid::launch_put_records(ix->mat, ix->rs, d_rec, w32_rec, colour_base / 32u, ix->w32, nr, ix->m, n_colors_total, d_err, c->stream);
    });
}

extern "C" {

int cid_index_put_records(cid_index *ix, const uint8_t *records, size_t n_records) {
    if (!ix) return fail(CID_ERR_INVALID, "null argument");
    return cid::index_put_records_slice(ix, records, n_records, ix->n_colors, 0);
}

// `merge`: file colour c -> index colour colour_map[c].  The map is increasing, so the file colours of one output word are one run;
// the plan lists the words the file reaches (k_put_records_mapped).  Only one upload chunk of records is on the device at a time.
int cid_index_put_records_mapped(cid_index *ix, const uint8_t *records, size_t n_records, uint32_t n_colors_file, const uint32_t *colour_map) {
    if (!ix || (n_records && !records) || !colour_map) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (n_colors_file == 0 || n_colors_file > ix->n_colors)
        return fail(CID_ERR_INVALID, "%u file colours into an index of %u", n_colors_file, ix->n_colors);
    std::vector<cid::MergePlan> plan;
    for (uint32_t c = 0; c < n_colors_file; ++c) {
        const uint32_t to = colour_map[c];
        if (to >= ix->n_colors) return fail(CID_ERR_INVALID, "colour_map[%u] = %u >= n_colors %u", c, to, ix->n_colors);
        if (c && to <= colour_map[c - 1]) return fail(CID_ERR_INVALID, "colour_map not strictly increasing at %u (%u after %u)", c, to, colour_map[c - 1]);
        if (plan.empty() || plan.back().w != to / 32u) plan.push_back(cid::MergePlan{to / 32u, c, 0u, 0u});
        plan.back().mask |= 1u << (to % 32u);
    }
    if (n_records == 0) return CID_OK;
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t w32_rec = (n_colors_file + 31u) / 32u;
    const uint32_t n_plan = (uint32_t)plan.size();
    void *d_plan;
    int rc = slot_reserve(c, S_ROWIDS, plan.size() * sizeof(cid::MergePlan), &d_plan);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(cid::MergePlan), hipMemcpyHostToDevice, c->stream));
    return stage_records(c, records, n_records, w32_rec, n_plan, [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
        return cid::launch_put_records_mapped(ix->mat, ix->rs, d_rec, w32_rec, (const cid::MergePlan *)d_plan, n_plan, nr, ix->m, n_colors_file,
                                              d_err, c->stream);
    });
}

// `subset`: the k-th set bit of keep_words (a bitmap over the file's colours) becomes index colour k.  The bitmap becomes a plan once per
// call: the file words that keep anything, and per output word where its 32 kept bits start among them (k_put_records_subset).  Rows are
// stored whole, so one file fills the index; only one upload chunk of records is on the device at a time.
int cid_index_put_records_subset(cid_index *ix, const uint8_t *records, size_t n_records, uint32_t n_colors_file, const uint32_t *keep_words) {
    if (!ix || (n_records && !records) || !keep_words) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (n_colors_file == 0) return fail(CID_ERR_INVALID, "a file of 0 colours");
    const uint32_t w32_rec = (n_colors_file + 31u) / 32u;
    if (keep_words[w32_rec - 1] & ~cid::tail_mask(n_colors_file))
        return fail(CID_ERR_INVALID, "keep bitmap has a bit at or beyond the file's %u colours", n_colors_file);
    std::vector<cid::SubsetItem> items;
    std::vector<uint64_t> before;   // kept bits before each item
    uint64_t kept = 0;
    for (uint32_t s = 0; s < w32_rec; ++s)
        if (keep_words[s]) {
            items.push_back(cid::SubsetItem{s, keep_words[s]});
            before.push_back(kept);
            kept += (uint64_t)__builtin_popcount(keep_words[s]);
        }
    if (kept != ix->n_colors) return fail(CID_ERR_INVALID, "keep bitmap selects %llu colours, the index has %u", (unsigned long long)kept, ix->n_colors);
    std::vector<cid::SubsetWord> words(ix->w32);
    for (uint32_t j = 0, first = 0; j < ix->w32; ++j) {
        const uint64_t lo = 32ull * j, hi = std::min<uint64_t>(lo + 32u, kept) - 1;   // the word's first and last kept bit
        while (first + 1 < items.size() && before[first + 1] <= lo) ++first;
        uint32_t last = first;
        while (last + 1 < items.size() && before[last + 1] <= hi) ++last;
        words[j] = cid::SubsetWord{first, (uint32_t)(lo - before[first]), last - first + 1, 0u};
    }
    if (n_records == 0) return CID_OK;
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t words_bytes = words.size() * sizeof(cid::SubsetWord), items_bytes = items.size() * sizeof(cid::SubsetItem);
    void *d_plan;
    int rc = slot_reserve(c, S_ROWIDS, words_bytes + items_bytes, &d_plan);   // the words (16 B each), then the items (8 B each)
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_plan, words.data(), words_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((uint8_t *)d_plan + words_bytes, items.data(), items_bytes, hipMemcpyHostToDevice, c->stream));
    return stage_records(c, records, n_records, w32_rec, ix->w32, [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
        return cid::launch_put_records_subset(ix->mat, ix->rs, d_rec, w32_rec, (const cid::SubsetWord *)d_plan,
                                              (const cid::SubsetItem *)((const uint8_t *)d_plan + words_bytes), ix->w32, nr, ix->m, n_colors_file,
                                              d_err, c->stream);
    });
}

// `fold`: bloom_size_file = factor x the index's bloom_size.  Each piece is checked on the device against the FILE's shape (k_pairs_check:
// row < bloom_size_file, word count, bit count, tail bits) before k_put_records_folded ORs it in, so a refused piece changes nothing.
int cid_index_put_records_folded(cid_index *ix, const uint8_t *records, size_t n_records, uint64_t bloom_size_file) {
    if (!ix || (n_records && !records)) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (cid::fold_factor(bloom_size_file, ix->m) == 0)
        return fail(CID_ERR_INVALID, "a file of bloom_size %llu does not fold onto %llu rows: not a multiple", (unsigned long long)bloom_size_file,
                    (unsigned long long)ix->m);
    if (n_records == 0) return CID_OK;
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    return stage_records(
        c, records, n_records, ix->w32, 1,
        [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
            return cid::launch_pairs_check(d_rec, ix->w32, nr, bloom_size_file, ix->n_colors, d_err, c->stream);
        },
        [&](const uint32_t *d_rec, size_t nr) {
            HIP_TRY(cid::launch_put_records_folded(ix->mat, ix->rs, d_rec, ix->w32, nr, ix->mod, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));   // the slot is the next piece's upload buffer
            return (int)CID_OK;
        });
}

// `collapse`: file colour c -> index colour group_of[c], any many-to-one map onto the index's colours; the plan is built once per call
// (cid_collapse.hpp).  Each piece is checked on the device against the FILE's shape (k_pairs_check) before k_put_records_grouped stores
// its rows and counts its columns, and the piece's counts are added to the caller's arrays when the piece is done: a refused piece
// changes neither the matrix nor the counters.  One slot holds the counters (zeroed before every piece), the plan's words and its items.
int cid_index_put_records_grouped(cid_index *ix, const uint8_t *records, size_t n_records, uint32_t n_colors_file, const uint32_t *group_of,
                                  uint64_t *bits_file, uint64_t *bits_index) {
    if (!ix || (n_records && !records) || !group_of) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (n_colors_file == 0) return fail(CID_ERR_INVALID, "a file of 0 colours");
    if (n_colors_file > (1u << 20)) return fail(CID_ERR_UNSUPPORTED, "a file of %u colours > 2^20", n_colors_file);
    std::vector<cid::GroupWord> words;
    std::vector<cid::GroupItem> items;
    uint32_t at = 0;
    switch (cid::build_group_plan(group_of, n_colors_file, ix->n_colors, words, items, at)) {
    case cid::kGroupPlanBeyond: return fail(CID_ERR_INVALID, "group_of[%u] = %u >= n_colors %u", at, group_of[at], ix->n_colors);
    case cid::kGroupPlanEmpty: return fail(CID_ERR_INVALID, "index colour %u has no member among the file's %u colours", at, n_colors_file);
    case cid::kGroupPlanOk: break;
    }
    if (n_records == 0) return CID_OK;
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool count = bits_file || bits_index;
    const size_t n_cnt = (size_t)n_colors_file + ix->n_colors;
    const size_t cnt_bytes = count ? (8 * n_cnt + 15) / 16 * 16 : 0, words_bytes = words.size() * sizeof(cid::GroupWord),
                 items_bytes = items.size() * sizeof(cid::GroupItem);
    void *d_plan;
    int rc = slot_reserve(c, S_ROWIDS, cnt_bytes + words_bytes + items_bytes, &d_plan);   // counters (8 B each), words (8 B), items (12 B)
    if (rc) return rc;
    uint8_t *d_words = (uint8_t *)d_plan + cnt_bytes;
    HIP_TRY(hipMemcpyAsync(d_words, words.data(), words_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_words + words_bytes, items.data(), items_bytes, hipMemcpyHostToDevice, c->stream));
    cid::GroupedParams p{};
    p.mat32 = reinterpret_cast<uint32_t *>(ix->mat); p.rs = ix->rs;
    p.w32_rec = (n_colors_file + 31u) / 32u; p.w32_out = ix->w32; p.n_colors_file = n_colors_file; p.n_colors = ix->n_colors;
    p.words = (const cid::GroupWord *)d_words; p.items = (const cid::GroupItem *)(d_words + words_bytes);
    p.counts = count ? (unsigned long long *)d_plan : nullptr;
    std::vector<uint64_t> got(count ? n_cnt : 0);
    // four threads a record (a workgroup of 256 walks tiles of 64): far from stage_records' thread cap
    return stage_records(
        c, records, n_records, p.w32_rec, 4,
        [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
            return cid::launch_pairs_check(d_rec, p.w32_rec, nr, ix->m, n_colors_file, d_err, c->stream);
        },
        [&](const uint32_t *d_rec, size_t nr) {
            if (count) HIP_TRY(hipMemsetAsync(d_plan, 0, 8 * n_cnt, c->stream));
            p.rec32 = d_rec; p.n_records = nr;
            HIP_TRY(cid::launch_put_records_grouped(p, c->n_cu, c->stream));
            if (count) HIP_TRY(hipMemcpyAsync(got.data(), d_plan, 8 * n_cnt, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));   // the slot is the next piece's upload buffer
            for (uint32_t f = 0; bits_file && f < n_colors_file; ++f) bits_file[f] += got[f];
            for (uint32_t g = 0; bits_index && g < ix->n_colors; ++g) bits_index[g] += got[n_colors_file + g];
            return (int)CID_OK;
        });
}

int cid_index_put_index_folded(cid_index *dst, const cid_index *src) {
    if (!dst || !src) return fail(CID_ERR_INVALID, "null argument");
    if (dst->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (!src->finalized) return fail(CID_ERR_INVALID, "source index not finalized");
    if (src->n_colors != dst->n_colors) return fail(CID_ERR_INVALID, "a source of %u colours into an index of %u", src->n_colors, dst->n_colors);
    cid_ctx *c = dst->ctx;
    if (src->ctx->device != c->device) return fail(CID_ERR_INVALID, "source index lives on device %d, the index on %d", src->ctx->device, c->device);
    const uint64_t factor = cid::fold_factor(src->m, dst->m);
    if (factor == 0)
        return fail(CID_ERR_INVALID, "a source of bloom_size %llu does not fold onto %llu rows: not a multiple", (unsigned long long)src->m,
                    (unsigned long long)dst->m);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(src->ctx->stream));   // (another ctx of the device may have filled the source)
    HIP_TRY(cid::launch_fold_rows(dst->mat, src->mat, dst->rs, dst->w32, dst->m, factor, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

int cid_index_device_matrix(cid_index *ix, void **dev_ptr, uint64_t *row_stride_words) {
    if (!ix || !dev_ptr || !row_stride_words) return fail(CID_ERR_INVALID, "null argument");
    *dev_ptr = ix->mat;
    *row_stride_words = ix->rs;
    return CID_OK;
}

int cid_index_finalize(cid_index *ix) {
    if (!ix) return fail(CID_ERR_INVALID, "null index");
    HIP_TRY(hipSetDevice(ix->ctx->device));
    HIP_TRY(hipStreamSynchronize(ix->ctx->stream));
    ix->finalized = true;
    return CID_OK;
}

int cid_index_get_rows(const cid_index *ix, const uint64_t *row_ids, uint32_t *words_le, size_t n_rows) {
    if (!ix || (n_rows && (!row_ids || !words_le))) return fail(CID_ERR_INVALID, "null argument");
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    for (size_t i = 0; i < n_rows; ++i)
        if (row_ids[i] >= ix->m) return fail(CID_ERR_INVALID, "row id %llu >= bloom_size", (unsigned long long)row_ids[i]);
    void *d_ids, *d_words;
    int rc = slot_reserve(c, S_ROWIDS, n_rows * 8, &d_ids);
    if (rc) return rc;
    rc = slot_reserve(c, S_WORDS, n_rows * ix->w32 * 4, &d_words);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_ids, row_ids, n_rows * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(cid::launch_get_rows(ix->mat, ix->rs, (const uint64_t *)d_ids, (uint32_t *)d_words, ix->w32, n_rows, c->stream));
    HIP_TRY(hipMemcpyAsync(words_le, d_words, n_rows * ix->w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

int cid_index_get_records(const cid_index *ix, uint64_t row_begin, uint64_t n_rows, uint8_t *records, uint64_t *n_records) {
    if (!ix || !n_records || (n_rows && !records)) return fail(CID_ERR_INVALID, "null argument");
    if (row_begin > ix->m || n_rows > ix->m - row_begin) return fail(CID_ERR_INVALID, "rows [%llu, +%llu) outside bloom_size",
                                                                     (unsigned long long)row_begin, (unsigned long long)n_rows);
    HIP_TRY(hipSetDevice(ix->ctx->device));
    return cid::index_get_records(ix->ctx, ix, row_begin, n_rows, records, n_records);
}

int cid_index_insert_kmers_dev(cid_index *ix, const uint8_t *d_kmers, const uint32_t *d_colour_of_kmer, size_t n_kmers) {
    if (!ix || (n_kmers && (!d_kmers || !d_colour_of_kmer))) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (!aligned16(d_kmers)) return fail(CID_ERR_INVALID, "d_kmers must be 16-byte aligned");
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    cid::InsertParams p = cid::insert_params(ix, n_kmers);
    p.kmers = d_kmers; p.colour_of_kmer = d_colour_of_kmer;
    HIP_TRY(cid::launch_insert_kmers(p, c->stream));
    return CID_OK;
}

int cid_index_insert_kmers(cid_index *ix, const uint8_t *kmers, uint32_t colour, size_t n_kmers) {
    if (!ix || (n_kmers && !kmers)) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (colour >= ix->n_colors) return fail(CID_ERR_INVALID, "colour %u >= n_colors", colour);
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    void *d_k;
    int rc = slot_reserve(c, S_KMERS, n_kmers * ix->k, &d_k);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_k, kmers, n_kmers * ix->k, hipMemcpyHostToDevice, c->stream));
    cid::InsertParams p = cid::insert_params(ix, n_kmers);
    p.kmers = (const uint8_t *)d_k; p.colour = colour;
    HIP_TRY(cid::launch_insert_kmers(p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

void cid_index_destroy(cid_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    (void)hipStreamSynchronize(ix->ctx->stream);
    if (ix->mat) (void)hipFree(ix->mat);
    delete ix;
}

int cid_index_row_stride_words(const cid_index *ix, uint64_t *row_stride_words) {
    if (!ix || !row_stride_words) return fail(CID_ERR_INVALID, "null argument");
    *row_stride_words = ix->rs;
    return CID_OK;
}

}  // extern "C"

namespace cid {
int index_insert_keys(cid_index *ix, const DevKeys &keys, uint32_t colour) {
    if (!ix || (keys.n && !keys.ascii && !keys.codes)) return fail(CID_ERR_INVALID, "null argument");
    if (ix->finalized) return fail(CID_ERR_STATE, "index already finalized");
    if (ix->k != keys.k) return fail(CID_ERR_INVALID, "k-mer set k=%u, index k=%u", keys.k, ix->k);
    if (colour >= ix->n_colors) return fail(CID_ERR_INVALID, "colour %u >= n_colors", colour);
    cid_ctx *c = ix->ctx;
    HIP_TRY(hipSetDevice(c->device));
    InsertParams p = insert_params(ix, keys.n);
    p.kmers = keys.ascii; p.codes = keys.codes; p.colour = colour;
    HIP_TRY(cid::launch_insert_kmers(p, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}
}  // namespace cid
