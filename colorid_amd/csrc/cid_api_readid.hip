// C ABI of libcolorid_hip.so, part 4: per-read classification counts — the body of read_id_mt_pe::parallel_vec before kmer_poll_plus
// (src/read_id_mt_pe.rs:300-331; search_index_classic :66-102, search_index :104-165), whole indices and colour stripes, dense and
// sparse reports.  Kernels: cid_readid.hip (reads that fit a wave's LDS) and cid_kmerset.hip (the sort-based long-read path).
#include "cid_api_common.hpp"

using cid::check_ready;
using cid::DevReads;
using cid::fail;
using cid::HostOffsets;
using cid::ReadOut;
using cid::slot_reserve;
using namespace cid::slots;

extern "C" {

// LDS layout of k_readid (bytes_kernel = false) or k_readid_bytes for reads of at most max_bytes bases / max_win windows;
// returns the bytes one wave needs (the kernels carve the same regions in the same order)
static size_t readid_layout(const cid_index *ix, uint32_t stride_d, uint32_t start_sample, uint64_t max_bytes, uint64_t max_win,
                            bool bytes_kernel, cid::ReadIdParams *pp, int slot_kind = 0 /* 0: key + index, 1: one u64, 2: one u32 position */) {
    // (pp == NULL: only the size is wanted — the routing asks once per read, and clearing a parameter block per question cost a
    // millisecond per hundred thousand reads)
    const bool packed_table = slot_kind == 1;
    if (max_bytes > (1ull << 30) || max_win > (1ull << 30)) return ~(size_t)0;
    const bool wide = ix->rs > 128;
    const uint32_t bases_cap = (uint32_t)((max_bytes + 16 + 15) & ~15ull);
    uint32_t win_cap = (uint32_t)((max_win + 3) & ~3ull);
    if (win_cap < 4) win_cap = 4;
    const uint32_t hist_pad = wide ? 4u * ix->rs : ((ix->n_colors + 1 + 3) & ~3u);   // wide rows: AND word + sampled-colour set
    uint32_t table_slots = 64;
    while (table_slots < win_cap + win_cap / 2) table_slots <<= 1;
    size_t slot_bytes = 12;
    uint32_t idx_bits = 0;
    if (packed_table) {   // one u64 per slot: code << idx_bits | window index
        uint32_t ib = 1;
        while ((1ull << ib) <= win_cap) ++ib;
        if (2u * ix->k + ib > 63u) return ~(size_t)0;
        idx_bits = ib;
        slot_bytes = 8;
    }
    if (slot_kind == 2) slot_bytes = 4;
    const size_t chunk_rows = 4ull * cid::kWave * ix->n_hash;                     // one chunk's row numbers
    const size_t rall_bytes = wide ? 0 : 4ull * win_cap * ix->n_hash;             // rows of the read's distinct k-mers (wide rows search chunk by chunk)
    // k_readid keeps no byte image of the read, but the raw bases of the NEXT one (LDS-DMA, one 16-byte piece per lane)
    const uint32_t stage_bytes = bytes_kernel ? 0u : std::min<uint32_t>(bases_cap, 16u * cid::kWave);
    size_t wave_bytes = (bytes_kernel ? (size_t)bases_cap : (size_t)stage_bytes) + rall_bytes;
    if (bytes_kernel)   // histogram, tags, window infos, k-mer image (+ minimizer image and the distinct minimizer strings)
        wave_bytes += 4ull * hist_pad + chunk_rows + 8ull * win_cap + cid::kmer_img_bytes(ix->k) +
                      (ix->m_size ? cid::kmer_img_bytes(ix->m_size) + (((size_t)win_cap * ix->m_size + 15) & ~15ull) : 0);
    else if (wide)      // chunk rows, histogram, hash table keys + indices, 2-bit bases, bad-base bits
        wave_bytes += chunk_rows + 4ull * hist_pad + 12ull * table_slots + 4ull * (bases_cap / 16 + 4) + 4ull * (bases_cap / 32 + 4);
    else                // the histogram shares the hash table's region (k_readid)
        wave_bytes += (CID_READID_ALIAS ? std::max<size_t>(slot_bytes * table_slots, 4ull * hist_pad) : slot_bytes * table_slots + 4ull * hist_pad) +
                      4ull * (bases_cap / 16 + 4) + 4ull * (bases_cap / 32 + 4);
    wave_bytes = (wave_bytes + 15) & ~15ull;
    if (pp) {
        cid::ReadIdParams &p = *pp;
        p = cid::ReadIdParams{};
        p.mat = ix->mat; p.rs = ix->rs; p.w64 = ix->w64; p.n_colors = ix->n_colors; p.n_hash = ix->n_hash; p.k = ix->k;
        p.mod = ix->mod;
        p.stride_d = stride_d; p.start_sample = start_sample;
        p.m_size = ix->m_size;
        p.bases_cap = bases_cap; p.win_cap = win_cap; p.hist_pad = hist_pad; p.table_slots = table_slots; p.idx_bits = idx_bits;
        p.slot4 = slot_kind == 2 ? 1u : 0u;
        p.stage_bytes = stage_bytes;
        p.wave_bytes = (uint32_t)(wave_bytes < 0xFFFFFFF0ull ? wave_bytes : 0xFFFFFFF0ull);
    }
    return wave_bytes;
}
// what a read needs of the LDS kernels: k <= 32 reads may end up in either of them
static size_t readid_need(const cid_index *ix, uint32_t stride_d, uint32_t start_sample, uint64_t max_bytes, uint64_t max_win) {
    const size_t b = readid_layout(ix, stride_d, start_sample, max_bytes, max_win, true, nullptr);
    if (ix->k > 32) return b;
    const size_t a = readid_layout(ix, stride_d, start_sample, max_bytes, max_win, false, nullptr);
    return a > b ? a : b;
}

constexpr size_t kLdsBytes = 160u * 1024u;
// device scratch for dense read_id report rows per launch: cid_readid_count slices larger batches, the sparse form refuses them
// (cid_ctx_tune "dense_report_bytes" / CID_DENSE_REPORT_BYTES: 2 GiB)
// k_readid keeps a read's set in one wave's LDS.  With fewer than six waves per CU its gathers are no longer hidden and the long-read
// path (cid_readlong.hip) is faster: 150 Mbases resident, configs[2]'s index, ms per call k_readid / long path (tools/exp_readlen_route.py,
// profiles/r06_readlen_route.jsonl): 300 bases 6.5 / 9.5, 600 bases 6.5 / 8.0, 800 bases (five waves) 8.7 / 7.7, 1000 bases (four waves)
// 12.9 / 7.5, 2000 bases 18.3 / 7.1.  (Round 5's long path took 10.4 at 800 bases: the rule then was "fewer than five waves"; round 1's
// sorting path took 20 ms whatever the length: "fewer than two".)
constexpr size_t kLdsReadBytesMax = kLdsBytes / 6;

static int readid_params(const cid_ctx *c, const cid_index *ix, uint32_t stride_d, uint32_t start_sample, uint64_t max_bytes, uint64_t max_win,
                         bool bytes_kernel, cid::ReadIdParams &p, int &waves, bool striped = false) {
    size_t wave_bytes = 0, best = 0;
    auto choose = [&](int slot_kind) {
        wave_bytes = readid_layout(ix, stride_d, start_sample, max_bytes, max_win, bytes_kernel, &p, slot_kind);
        // waves per workgroup: whatever puts the most waves on a CU (160 KiB of LDS, at most 8 workgroups of this size... 32 waves)
        waves = 1;
        best = 0;
        if (wave_bytes == ~(size_t)0) return;
        for (int w = 4; w >= 1; --w) {
            if ((size_t)w * wave_bytes > kLdsBytes) continue;
            size_t blocks = kLdsBytes / ((size_t)w * wave_bytes);
            if (blocks > 32u / (size_t)w) blocks = 32u / (size_t)w;
            if (blocks * (size_t)w > best) { best = blocks * (size_t)w; waves = w; }
        }
    };
    // the 8-byte-per-slot set is built for the six-waves-per-SIMD kernel only (whole k-mers, published hash, rows <= 1 KiB, no stripe
    // passes): taken when the 12-byte slots leave fewer than six waves per SIMD and the 8-byte ones reach them (paired 150-bp reads,
    // k <= 27: 10.6 -> 10.1 ms per million pairs, tools/exp_readid_table.py)
    const bool can_pack = !bytes_kernel && c->tune.readid_packed_table && ix->rs <= 128 && !ix->m_size && ix->k <= 31 &&
                          ((ix->mod.flags >> 8) & 0xFFu) == CID_HASH_XXH3_V08 && !striped;
    // ... and where the code leaves no room for the index (k = 28..32) the slot holds a position only (4 bytes; the probe reads the k-mer back)
    const bool can_slot4 = !bytes_kernel && c->tune.readid_packed_table && ix->rs <= 128 && !ix->m_size && ix->k <= 32 &&
                           ((ix->mod.flags >> 8) & 0xFFu) == CID_HASH_XXH3_V08 && !striped;
    choose(0);
    if (best < 24 && (can_pack || can_slot4)) {   // (where six waves per SIMD fit anyway the 12-byte slots are marginally faster: 6.02 vs 6.07 ms single-end)
        const size_t classic = best;
        if (can_pack) choose(1);
        if ((!can_pack || wave_bytes == ~(size_t)0 || best < 24) && can_slot4) choose(2);
        if (best <= classic || best <= 20) choose(0);   // worth it only with more waves than the 96-VGPR (5 per SIMD) build runs
    }
    if (wave_bytes > kLdsBytes)
        return fail(CID_ERR_UNSUPPORTED, "a read(-pair) of %llu bases / %llu windows needs %zu B of LDS per wave (> 160 KiB): "
                    "use the host-pointer calls, which route such reads through the sort-based path", (unsigned long long)max_bytes,
                    (unsigned long long)max_win, wave_bytes);
    return CID_OK;
}

using StripeArgs = cid::StripePass;

static int readid_dev_impl(cid_ctx *c, const cid_index *ix, const DevReads &b, uint64_t max_read_bytes, uint64_t max_read_windows, const uint8_t *d_skip,
                           bool clear_wide, const ReadOut &o, const StripeArgs &sa = StripeArgs()) {
    const size_t n_reads = b.n_reads;
    const uint32_t stride_d = b.stride_d, start_sample = b.start_sample;
    if (n_reads >= (1ull << 32)) return fail(CID_ERR_UNSUPPORTED, "more than 2^32 reads in one batch");
    cid::ReadIdParams pb, pp;
    int waves_b, waves_p = 0;
    int rc = readid_params(c, ix, stride_d, start_sample, max_read_bytes, max_read_windows, true, pb, waves_b);
    if (rc) return rc;
    const bool packable = ix->k <= 32;
    const bool striped = sa.zero_acc || sa.zero_in;
    if (packable && (rc = readid_params(c, ix, stride_d, start_sample, max_read_bytes, max_read_windows, false, pp, waves_p, striped))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    auto fill = [&](cid::ReadIdParams &p, int waves) {
        p.bases = b.d_bases; p.seq_off = b.d_seq_off; p.read_seq0 = b.d_read_seq0; p.n_reads = n_reads;
        p.report = o.d_report; p.n_kmers = o.d_n_kmers; p.status = o.d_status; p.skip = d_skip;
        p.zero_acc = sa.zero_acc; p.zero_in = sa.zero_in; p.zero_start = sa.zero_start;
        p.colour_base = sa.colour_base; p.report_width = sa.report_width; p.write_nohits = sa.write_nohits;
        uint64_t rpb = n_reads / ((uint64_t)c->n_cu * (uint64_t)c->tune.readid_blocks_per_cu);   // (16 -> 64 per CU: -3 %, the tail of the grid)
        if (rpb < (uint64_t)waves) rpb = waves;
        if (rpb > 256) rpb = 256;
        p.reads_per_block = (uint32_t)rpb;
    };
    if (ix->rs > 128 && clear_wide)   // wide rows count in place
        HIP_TRY(hipMemsetAsync(o.d_report, 0, n_reads * ((size_t)ix->n_colors + 1) * 4, c->stream));
    if (!d_skip) {   // device-pointer callers state the maxima: reads beyond them are marked and left alone (k_readid_check_caps)
        void *d_sk;
        rc = slot_reserve(c, S_ROUTE, n_reads, &d_sk); if (rc) return rc;
        cid::ReadIdParams pc = pb;   // bases_cap / win_cap are the same for both kernels' layouts
        fill(pc, waves_b);
        pc.report_width = (sa.zero_acc || sa.zero_in) ? 0u : ix->n_colors + 1;   // striped passes only add to rows the caller zeroed
        HIP_TRY(cid::launch_readid_check_caps(pc, (uint8_t *)d_sk, c->stream));
        d_skip = (const uint8_t *)d_sk;
    }
    if (packable) {
        // k_readid takes every read it can pack; the ones with lower-case bases come back in the redo list for k_readid_bytes
        void *d_redo;
        rc = slot_reserve(c, S_REDO, 16 + 4 * n_reads, &d_redo); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_redo, 0, 16, c->stream));
        fill(pp, waves_p);
        pp.redo_count = (uint32_t *)d_redo; pp.redo_list = (uint32_t *)d_redo + 4;
        HIP_TRY(cid::launch_readid(pp, waves_p, c->stream));
        fill(pb, waves_b);
        pb.redo_count = pp.redo_count; pb.redo_list = pp.redo_list;
        uint64_t grid = (n_reads + waves_b - 1) / waves_b;
        if (grid > (uint64_t)c->n_cu * 4) grid = (uint64_t)c->n_cu * 4;
        HIP_TRY(cid::launch_readid_bytes(pb, waves_b, (int)grid, c->stream));
    } else {
        fill(pb, waves_b);
        uint64_t grid = (n_reads + waves_b - 1) / waves_b;
        if (grid > (uint64_t)c->n_cu * 64) grid = (uint64_t)c->n_cu * 64;
        HIP_TRY(cid::launch_readid_bytes(pb, waves_b, (int)grid, c->stream));
    }
    return CID_OK;
}

// Which kernel takes which read of a batch.  Reads of at least long_from(...) bases take the long-read path (cid_readlong.hip), the others
// the LDS kernels.  The rule is a threshold on a read's bases alone, so that the device applies it to offsets that never exist on the
// host (cid::long_route_launch): the smallest read whose set — with the windows a read of that many bases has, (bases - k) / stride + 1 —
// would leave k_readid fewer than six waves per CU (kLdsReadBytesMax).  cid_ctx_tune "readid_long_from" = L: every read of at least L
// bases does (measurements).
static uint64_t long_from(const cid_ctx *c, const cid_index *ix, uint32_t stride_d, uint32_t start_sample) {
    if (c->tune.readid_long_from >= 0) return (uint64_t)c->tune.readid_long_from;
    auto need = [&](uint64_t b) { return readid_need(ix, stride_d, start_sample, b, b >= ix->k ? (b - ix->k) / stride_d + 1 : 0); };
    uint64_t lo = 0, hi = 1ull << 21;   // need(lo) fits, need(hi) does not
    if (need(hi) <= kLdsReadBytesMax) return ~0ull;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (need(mid) <= kLdsReadBytesMax) lo = mid; else hi = mid;
    }
    return hi;
}
// A batch with long reads, everything on the device: the route (d_route: S_ROUTE), the long-read path for its reads, the LDS kernels for the
// rest.  cap_*: the maxima a device-pointer caller stated (reads beyond them: status 3), ~0 = none.  host: the offsets on the host, or NULL.
static int readid_routed(cid_ctx *c, const cid_index *ix, const DevReads &b, uint64_t cap_bytes, uint64_t cap_win, bool clear_wide, const ReadOut &o,
                         const StripeArgs &sa, const HostOffsets *host) {
    int rc;
    void *d_route;
    const size_t n_reads = b.n_reads;
    if ((rc = slot_reserve(c, S_ROUTE, n_reads + 16 + 16, &d_route))) return rc;
    uint32_t *d_stats = reinterpret_cast<uint32_t *>((uint8_t *)d_route + ((n_reads + 15) & ~(size_t)15));
    if ((rc = cid::long_route_launch(c, b, ix->k, long_from(c, ix, b.stride_d, b.start_sample), cap_bytes, cap_win, (uint8_t *)d_route, d_stats))) return rc;
    const bool striped = sa.on();
    const size_t C1 = (size_t)ix->n_colors + 1;
    // wide rows count in place, and both kernels add into the same report: cleared once, here
    if (ix->rs > 128 && clear_wide && !striped) HIP_TRY(hipMemsetAsync(o.d_report, 0, n_reads * C1 * 4, c->stream));
    uint32_t stats[4] = {0, 0, 0, 0};
    // first: it writes a status for every read (2 = the other kernels')
    if ((rc = cid::readid_long(c, ix, b, (const uint8_t *)d_route, false, o, sa, host, d_stats, stats))) return rc;
    if (stats[1])   // the reads of the LDS kernels, sized by the longest of THEM
        if ((rc = readid_dev_impl(c, ix, b, stats[2], stats[3] ? stats[3] : 1, (const uint8_t *)d_route, false, o, sa))) return rc;
    if (cap_bytes != ~0ull || cap_win != ~0ull)
        if ((rc = cid::long_beyond_launch(c, (const uint8_t *)d_route, n_reads, striped ? 0u : (uint32_t)C1, o))) return rc;
    return CID_OK;
}

int cid_readid_count_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *d_seq_off,
                         const uint64_t *d_read_seq0, size_t n_reads, uint32_t stride_d, uint32_t start_sample,
                         uint64_t max_read_bytes, uint64_t max_read_windows, uint32_t *d_report, uint32_t *d_n_kmers,
                         uint8_t *d_status) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (stride_d == 0) return fail(CID_ERR_INVALID, "stride_d must be >= 1");
    if (n_reads == 0) return CID_OK;
    if (!d_bases || !d_seq_off || !d_read_seq0 || !d_report || !d_n_kmers || !d_status) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const DevReads b{.d_bases = d_bases, .d_seq_off = d_seq_off, .d_read_seq0 = d_read_seq0, .n_reads = n_reads, .stride_d = stride_d,
                     .start_sample = start_sample};
    const ReadOut o{.d_report = d_report, .d_n_kmers = d_n_kmers, .d_status = d_status};
    if (max_read_bytes >= long_from(c, ix, stride_d, start_sample))   // reads of any length: the long ones through cid_readlong.hip, in the same call
        return readid_routed(c, ix, b, max_read_bytes, max_read_windows, true, o, StripeArgs(), nullptr);
    return readid_dev_impl(c, ix, b, max_read_bytes, max_read_windows, nullptr, true, o);
}

// read_id over colour stripes (src/read_id_mt_pe.rs:66-165 with the absent-row stop decided over ALL colours).
// Pass 1, once per stripe: d_zero_acc[read * max_read_windows + q] &= the seeds whose row is all-zero in this stripe, for the
// read's q-th distinct k-mer (first-occurrence order).  Between the passes the caller ANDs the arrays of different GPUs.
// Pass 2, once per stripe: the ordered count; a k-mer is "absent" iff its accumulated mask is non-zero.
__global__ void k_mask_starts(uint64_t *zero_start, uint64_t n_reads, uint64_t stride) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_reads) zero_start[r] = r * stride;
}
// the device-pointer pair: masks laid out [read][max_read_windows]
static int readid_stripe_common(cid_ctx *c, const cid_index *ix, const void *d_bases, const void *d_seq_off, const void *d_read_seq0,
                                size_t n_reads, uint32_t stride_d, uint64_t max_read_bytes, uint64_t max_read_windows, const uint64_t **d_zero_start) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if (!d_bases || !d_seq_off || !d_read_seq0) return fail(CID_ERR_INVALID, "null argument");
    if (max_read_windows == 0 || max_read_windows > (1u << 20)) return fail(CID_ERR_INVALID, "max_read_windows out of range");
    if (readid_need(ix, 1, 0, max_read_bytes, max_read_windows) > kLdsBytes)
        return fail(CID_ERR_UNSUPPORTED,
                    "reads of %llu bases do not fit a wave's LDS: cid_readid_stripe_zero / _count route such reads through the sort-based path",
                    (unsigned long long)max_read_bytes);
    if (stride_d == 0) return fail(CID_ERR_INVALID, "stride_d must be >= 1");
    *d_zero_start = nullptr;
    if (n_reads == 0) return CID_OK;
    HIP_TRY(hipSetDevice(c->device));
    void *d_zs;
    rc = slot_reserve(c, S_ZSTART, n_reads * 8, &d_zs); if (rc) return rc;
    hipLaunchKernelGGL(k_mask_starts, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, c->stream, (uint64_t *)d_zs, (uint64_t)n_reads, max_read_windows);
    HIP_TRY(hipGetLastError());
    *d_zero_start = (const uint64_t *)d_zs;
    return CID_OK;
}

int cid_readid_stripe_zero_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *d_seq_off, const uint64_t *d_read_seq0,
                               size_t n_reads, uint32_t stride_d, uint64_t max_read_bytes, uint64_t max_read_windows, uint32_t *d_zero_acc,
                               uint32_t *d_n_kmers, uint8_t *d_status) {
    const uint64_t *d_zs;
    int rc = readid_stripe_common(c, ix, d_bases, d_seq_off, d_read_seq0, n_reads, stride_d, max_read_bytes, max_read_windows, &d_zs);
    if (rc) return rc;
    if (n_reads == 0) return CID_OK;
    if (!d_zero_acc || !d_n_kmers || !d_status) return fail(CID_ERR_INVALID, "null argument");
    StripeArgs sa;
    sa.zero_acc = d_zero_acc; sa.zero_start = d_zs; sa.report_width = ix->n_colors + 1;
    const DevReads b{.d_bases = d_bases, .d_seq_off = d_seq_off, .d_read_seq0 = d_read_seq0, .n_reads = n_reads, .stride_d = stride_d, .start_sample = 0};
    const ReadOut o{.d_report = d_zero_acc /* never written in this pass */, .d_n_kmers = d_n_kmers, .d_status = d_status};
    return readid_dev_impl(c, ix, b, max_read_bytes, max_read_windows, nullptr, false, o, sa);
}

int cid_readid_stripe_count_dev(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *d_seq_off, const uint64_t *d_read_seq0,
                                size_t n_reads, uint32_t stride_d, uint32_t start_sample, uint64_t max_read_bytes, uint64_t max_read_windows,
                                uint32_t colour_base, uint32_t n_colors_total, int write_nohits, const uint32_t *d_zero_acc, uint32_t *d_report,
                                uint32_t *d_n_kmers, uint8_t *d_status) {
    const uint64_t *d_zs;
    int rc = readid_stripe_common(c, ix, d_bases, d_seq_off, d_read_seq0, n_reads, stride_d, max_read_bytes, max_read_windows, &d_zs);
    if (rc) return rc;
    if ((uint64_t)colour_base + ix->n_colors > n_colors_total) return fail(CID_ERR_INVALID, "stripe [%u, +%u) outside %u colours", colour_base,
                                                                           ix->n_colors, n_colors_total);
    if (n_reads == 0) return CID_OK;
    if (!d_zero_acc || !d_report || !d_n_kmers || !d_status) return fail(CID_ERR_INVALID, "null argument");
    StripeArgs sa;
    sa.zero_in = d_zero_acc; sa.zero_start = d_zs; sa.colour_base = colour_base; sa.report_width = n_colors_total + 1;
    sa.write_nohits = write_nohits ? 1u : 0u;
    const DevReads b{.d_bases = d_bases, .d_seq_off = d_seq_off, .d_read_seq0 = d_read_seq0, .n_reads = n_reads, .stride_d = stride_d,
                     .start_sample = start_sample};
    const ReadOut o{.d_report = d_report, .d_n_kmers = d_n_kmers, .d_status = d_status};
    return readid_dev_impl(c, ix, b, max_read_bytes, max_read_windows, nullptr, false, o, sa);
}

// The two stripe passes for ANY read length and stripe width: d_bases resident, offsets on the host.  Per stripe the reads are routed
// between the LDS kernels and the sort-based path exactly as cid_readid_count routes them (the mask of a read's q-th distinct k-mer
// sits at the same word whichever kernel writes it, so different stripes may route a read differently).  Masks: one word per
// window, read r's at [prefix of the windows of reads 0..r-1] (cid_readid_stripe_mask_words words in all).
int cid_readid_stripe_mask_words(uint32_t k_size, uint32_t stride_d, const uint64_t *seq_off, const uint64_t *read_seq0, size_t n_reads, uint64_t *n_words) {
    if (!seq_off || !read_seq0 || !n_words) return fail(CID_ERR_INVALID, "null argument");
    if (stride_d == 0 || k_size == 0) return fail(CID_ERR_INVALID, "k_size and stride_d must be >= 1");
    const HostOffsets h{.seq_off = seq_off, .n_seqs = ~0ull /* the caller vouches for seq_off's length */, .read_seq0 = read_seq0, .n_reads = n_reads};
    const cid::BatchSizes z = cid::walk_batch(h, k_size, stride_d);
    if (const int rc = cid::batch_fail(z.fault)) return rc;
    *n_words = z.total_win + 1;   // never empty
    return CID_OK;
}

static int readid_stripe_pass(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const HostOffsets &h, uint32_t stride_d, uint32_t start_sample,
                              StripeArgs sa, const ReadOut &o) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = cid::check_batch(h, stride_d, d_bases))) return rc;
    const size_t n_reads = h.n_reads, n_seqs = h.n_seqs;
    if (n_reads == 0) return CID_OK;
    if (!o.d_n_kmers || !o.d_status) return fail(CID_ERR_INVALID, "null argument");
    std::vector<uint64_t> zs(n_reads + 1);
    const cid::BatchSizes z = cid::walk_batch(h, ix->k, stride_d, zs.data());   // the one walk: refused, or the sizes and the masks' starts
    if ((rc = cid::batch_fail(z.fault))) return rc;
    if (z.total_win >= (1ull << 32)) return fail(CID_ERR_UNSUPPORTED, "more than 2^32 k-mer windows in one read_id batch");
    HIP_TRY(hipSetDevice(c->device));
    void *d_so, *d_r0, *d_zs;
    const size_t b0 = (n_seqs + 1) * 8, b1 = (n_reads + 1) * 8;
    if ((rc = slot_reserve(c, S_SEQOFF, b0, &d_so)) || (rc = slot_reserve(c, S_READ0, b1, &d_r0)) || (rc = slot_reserve(c, S_ZSTART, b1, &d_zs))) return rc;
    if ((rc = cid::staged_upload(c, {{d_so, h.seq_off, b0}, {d_r0, h.read_seq0, b1}, {d_zs, zs.data(), b1}}, b0 + 2 * b1 + 64))) return rc;
    sa.zero_start = (const uint64_t *)d_zs;
    const DevReads b{.d_bases = d_bases, .d_seq_off = (const uint64_t *)d_so, .d_read_seq0 = (const uint64_t *)d_r0, .n_reads = n_reads,
                     .stride_d = stride_d, .start_sample = start_sample};
    if (z.max_bases >= long_from(c, ix, stride_d, start_sample))   // (the mask of a read's q-th distinct k-mer sits at the same word whichever kernel writes it)
        rc = readid_routed(c, ix, b, ~0ull, ~0ull, false, o, sa, &h);
    else
        rc = readid_dev_impl(c, ix, b, z.max_bases, z.max_win ? z.max_win : 1, nullptr, false, o, sa);
    HIP_TRY(hipStreamSynchronize(c->stream));   // the host vectors leave scope
    return rc;
}

int cid_readid_stripe_zero(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *seq_off, size_t n_seqs, const uint64_t *read_seq0,
                           size_t n_reads, uint32_t stride_d, uint32_t *d_zero_acc, uint32_t *d_n_kmers, uint8_t *d_status) {
    if (n_reads && !d_zero_acc) return fail(CID_ERR_INVALID, "null argument");
    StripeArgs sa;
    sa.zero_acc = d_zero_acc; sa.report_width = ix ? ix->n_colors + 1 : 0;
    const HostOffsets h{.seq_off = seq_off, .n_seqs = n_seqs, .read_seq0 = read_seq0, .n_reads = n_reads};
    const ReadOut o{.d_report = d_zero_acc /* never written in this pass */, .d_n_kmers = d_n_kmers, .d_status = d_status};
    return readid_stripe_pass(c, ix, d_bases, h, stride_d, 0, sa, o);
}

int cid_readid_stripe_count(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *seq_off, size_t n_seqs, const uint64_t *read_seq0,
                            size_t n_reads, uint32_t stride_d, uint32_t start_sample, uint32_t colour_base, uint32_t n_colors_total, int write_nohits,
                            const uint32_t *d_zero_acc, uint32_t *d_report, uint32_t *d_n_kmers, uint8_t *d_status) {
    if (n_reads && (!d_zero_acc || !d_report)) return fail(CID_ERR_INVALID, "null argument");
    if (ix && (uint64_t)colour_base + ix->n_colors > n_colors_total) return fail(CID_ERR_INVALID, "stripe [%u, +%u) outside %u colours", colour_base,
        ix->n_colors, n_colors_total);
    StripeArgs sa;
    sa.zero_in = d_zero_acc; sa.colour_base = colour_base; sa.report_width = n_colors_total + 1; sa.write_nohits = write_nohits ? 1u : 0u;
    const HostOffsets h{.seq_off = seq_off, .n_seqs = n_seqs, .read_seq0 = read_seq0, .n_reads = n_reads};
    const ReadOut o{.d_report = d_report, .d_n_kmers = d_n_kmers, .d_status = d_status};
    return readid_stripe_pass(c, ix, d_bases, h, stride_d, start_sample, sa, o);
}

// bases resident, offsets on the host: routes every read between the LDS kernels and the long-read path, uploads the offsets,
// runs the kernels into the caller's device arrays.  b.d_seq_off / b.d_read_seq0 non-null: the offsets are on the device already (the
// caller uploaded them together with the bases).
static int readid_resident(cid_ctx *c, const cid_index *ix, DevReads b, const HostOffsets &h, const ReadOut &o) {
    const cid::BatchSizes z = cid::walk_batch(h, ix->k, b.stride_d);
    int rc = cid::batch_fail(z.fault);
    if (rc) return rc;
    if (!b.d_seq_off) {
        void *d_so, *d_r0;
        const size_t b0 = (h.n_seqs + 1) * 8, b1 = (h.n_reads + 1) * 8;
        if ((rc = slot_reserve(c, S_SEQOFF, b0, &d_so)) || (rc = slot_reserve(c, S_READ0, b1, &d_r0))) return rc;
        if ((rc = cid::staged_upload(c, {{d_so, h.seq_off, b0}, {d_r0, h.read_seq0, b1}}, b0 + b1 + 64))) return rc;
        b.d_seq_off = (const uint64_t *)d_so; b.d_read_seq0 = (const uint64_t *)d_r0;
    }
    // any long read: the device routes every read between the long-read path and the LDS kernels and makes the former's work lists
    if (z.max_bases >= long_from(c, ix, b.stride_d, b.start_sample))
        return readid_routed(c, ix, b, ~0ull, ~0ull, true, o, StripeArgs(), &h);
    return readid_dev_impl(c, ix, b, z.max_bases, z.max_win ? z.max_win : 1, nullptr, true, o);
}

int cid_readid_count_resident(cid_ctx *c, const cid_index *ix, const uint8_t *d_bases, const uint64_t *seq_off, size_t n_seqs,
                              const uint64_t *read_seq0, size_t n_reads, uint32_t stride_d, uint32_t start_sample, uint32_t *d_report,
                              uint32_t *d_n_kmers, uint8_t *d_status) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    const HostOffsets h{.seq_off = seq_off, .n_seqs = n_seqs, .read_seq0 = read_seq0, .n_reads = n_reads};
    if ((rc = cid::check_batch(h, stride_d, d_bases))) return rc;
    if (n_reads == 0) return CID_OK;
    if (!d_report || !d_n_kmers || !d_status) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const DevReads b{.d_bases = d_bases, .d_seq_off = nullptr, .d_read_seq0 = nullptr, .n_reads = n_reads, .stride_d = stride_d, .start_sample = start_sample};
    const ReadOut o{.d_report = d_report, .d_n_kmers = d_n_kmers, .d_status = d_status};
    return readid_resident(c, ix, b, h, o);
}

// uploads the batch (n_reads > 0), runs the LDS kernels or the long-read path; leaves report / n_kmers / status in the ctx's device scratch
static int readid_to_device(cid_ctx *c, const cid_index *ix, const uint8_t *bases, const HostOffsets &h, uint32_t stride_d, uint32_t start_sample,
                            ReadOut &o) {
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = cid::check_batch(h, stride_d, bases))) return rc;
    const size_t n_seqs = h.n_seqs, n_reads = h.n_reads;
    const uint64_t total_bases = h.seq_off[n_seqs];
    HIP_TRY(hipSetDevice(c->device));
    void *d_bases, *d_so, *d_r0, *d_rep, *d_nk;
    const size_t C1 = (size_t)ix->n_colors + 1;
    const size_t b_so = (n_seqs + 1) * 8, b_r0 = (n_reads + 1) * 8;
    if ((rc = slot_reserve(c, S_BASES, total_bases, &d_bases)) || (rc = slot_reserve(c, S_SEQOFF, b_so, &d_so)) || (rc = slot_reserve(c, S_READ0, b_r0, &d_r0)) ||
        (rc = slot_reserve(c, S_REPORT, n_reads * C1 * 4, &d_rep)) || (rc = slot_reserve(c, S_NK, n_reads * 4 + n_reads + 16, &d_nk)))
        return rc;
    // Bases that lie in page-locked memory already (cid_pinned_alloc: the CLI's batches of long reads) travel from where they are: staged,
    // 48 MB of them were 10 ms of memcpy on the calling thread before 2 ms on the bus.
    bool bases_locked = false;
    if (total_bases >= ((size_t)4 << 20)) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, bases) == hipSuccess) bases_locked = at.type == hipMemoryTypeHost;
        else (void)hipGetLastError();   // (memory the runtime has never seen: not an error of this call)
    }
    // the rest goes through the ctx's pinned arena when it fits; the arena's tail is left for the results
    const size_t staged_bases = bases_locked ? 0 : total_bases;
    if ((rc = cid::staged_upload(c, {{d_bases, bases, staged_bases}, {d_so, h.seq_off, b_so}, {d_r0, h.read_seq0, b_r0}},
                                 ((staged_bases + 15) & ~(size_t)15) + b_so + b_r0 + n_reads * 5 + 64)))
        return rc;
    if (bases_locked) HIP_TRY(hipMemcpyAsync(d_bases, bases, total_bases, hipMemcpyHostToDevice, c->stream));
    o = ReadOut{.d_report = (uint32_t *)d_rep, .d_n_kmers = (uint32_t *)d_nk, .d_status = (uint8_t *)d_nk + n_reads * 4};
    const DevReads b{.d_bases = (const uint8_t *)d_bases, .d_seq_off = (const uint64_t *)d_so, .d_read_seq0 = (const uint64_t *)d_r0, .n_reads = n_reads,
                     .stride_d = stride_d, .start_sample = start_sample};
    return readid_resident(c, ix, b, h, o);
}

int cid_readid_count(cid_ctx *c, const cid_index *ix, const uint8_t *bases, const uint64_t *seq_off, size_t n_seqs,
                     const uint64_t *read_seq0, size_t n_reads, uint32_t stride_d, uint32_t start_sample,
                     uint32_t *report, uint32_t *n_kmers, uint8_t *status) {
    if (n_reads == 0) return check_ready(c, ix);
    if (!report || !n_kmers || !status) return fail(CID_ERR_INVALID, "null argument");
    if (!c || !ix || !seq_off || !read_seq0) return fail(CID_ERR_INVALID, "null argument");
    // A dense report row has n_colors+1 counters (4 GB per million reads at 1024 colours): the batch is worked through in
    // slices whose rows fit kDenseReportBytes of device scratch; a read's row does not depend on its neighbours.
    const size_t C1 = (size_t)ix->n_colors + 1;
    size_t per = (size_t)c->tune.dense_report_bytes / (C1 * 4);
    if (per == 0) per = 1;
    const HostOffsets whole{.seq_off = seq_off, .n_seqs = n_seqs, .read_seq0 = read_seq0, .n_reads = n_reads};
    std::vector<uint64_t> so, r0v;
    for (size_t r0 = 0; r0 < n_reads; r0 += per) {
        const size_t nr = n_reads - r0 < per ? n_reads - r0 : per;
        HostOffsets h = whole;
        const uint8_t *bases_p = bases;
        if (nr != n_reads) {   // the slice with its own seq_off / read_seq0 starting at 0
            uint64_t base;
            if (int rc = cid::batch_fail(cid::rebase_batch(whole, r0, r0 + nr, so, r0v, &base))) return rc;
            h = HostOffsets{.seq_off = so.data(), .n_seqs = so.size() - 1, .read_seq0 = r0v.data(), .n_reads = nr};
            bases_p = bases ? bases + base : nullptr;
        }
        ReadOut d;
        int rc = readid_to_device(c, ix, bases_p, h, stride_d, start_sample, d);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(report + r0 * C1, d.d_report, nr * C1 * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(n_kmers + r0, d.d_n_kmers, nr * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(status + r0, d.d_status, nr, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CID_OK;
}

int cid_readid_count_sparse(cid_ctx *c, const cid_index *ix, const uint8_t *bases, const uint64_t *seq_off, size_t n_seqs,
                            const uint64_t *read_seq0, size_t n_reads, uint32_t stride_d, uint32_t start_sample,
                            uint32_t *n_kmers, uint8_t *status, uint64_t *n_entries) {
    if (!n_entries) return fail(CID_ERR_INVALID, "null argument");
    *n_entries = 0;
    if (n_reads == 0) { int rc0 = check_ready(c, ix); if (rc0 == CID_OK) { c->sp_rows = 0; c->sp_entries = 0; } return rc0; }
    if (!n_kmers || !status) return fail(CID_ERR_INVALID, "null argument");
    if (ix && (double)n_reads * ((double)ix->n_colors + 1.0) * 4.0 > 64.0 * (double)(1ull << 30))
        return fail(CID_ERR_UNSUPPORTED, "%zu reads x %u colours need more than 64 GiB of dense report rows on the device: use smaller batches",
                    n_reads, ix->n_colors);
    ReadOut d;
    const HostOffsets h{.seq_off = seq_off, .n_seqs = n_seqs, .read_seq0 = read_seq0, .n_reads = n_reads};
    int rc = readid_to_device(c, ix, bases, h, stride_d, start_sample, d);
    if (rc) return rc;
    if ((rc = cid::store_sparse(c, d.d_report, ix->n_colors + 1, n_reads))) return rc;
    // (inputs are on the device by now: the arena is free again)
    if ((rc = cid::staged_download(c, {{n_kmers, d.d_n_kmers, n_reads * 4}, {status, d.d_status, n_reads}}, n_reads * 5 + 64))) return rc;
    *n_entries = c->sp_entries;
    return CID_OK;
}

int cid_readid_sparse_fetch(cid_ctx *c, uint64_t *row_start, uint32_t *colours, uint32_t *counts) {
    if (!c || !row_start) return fail(CID_ERR_INVALID, "null argument");
    if (c->sp_rows == 0) { row_start[0] = 0; return CID_OK; }
    if (c->sp_entries && (!colours || !counts)) return fail(CID_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t b_rs = (c->sp_rows + 1) * 8, b_e = c->sp_entries * 4;
    return cid::staged_download(c, {{row_start, c->sp_start, b_rs}, {colours, c->sp_col, b_e}, {counts, c->sp_cnt, b_e}}, b_rs + 2 * b_e + 64);
}
}  // extern "C"
