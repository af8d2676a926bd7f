// C ABI of libcolorid_hip.so, part 7: the greedy cover of a query by accessions (cid_search_gather, cid_search_gather_set).
// Kernels: cid_cover.hip (k_cover_rows, shared with the coverage search) and cid_gather_cover.hip.
#include "cid_api_common.hpp"

using cid::check_not_mini;
using cid::check_ready;
using cid::fail;
using cid::slot_reserve;
using namespace cid::slots;

namespace {

// device scratch of one call from the ctx's block cache; everything goes back when the call ends, whichever way
struct Scratch {
    cid_ctx *c;
    std::vector<void *> held;
    explicit Scratch(cid_ctx *ctx) : c(ctx) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { for (void *p : held) cid::ctx_free(c, p); }
    template <class T>
    int get(size_t n, T **out) {
        void *p = nullptr;
        const int rc = cid::ctx_alloc(c, (n ? n : 1) * sizeof(T), &p);
        if (rc) return rc;
        held.push_back(p);
        *out = static_cast<T *>(p);
        return CID_OK;
    }
};

int check_gather_args(const cid_ctx *c, const cid_index *ix, uint64_t min_new, const cid_gather_row *out, const size_t *n_out, const uint64_t *n_hit) {
    if (!out || !n_out || !n_hit) return fail(CID_ERR_INVALID, "null argument");
    if (min_new == 0) return fail(CID_ERR_INVALID, "min_new must be at least 1");
    int rc = check_ready(c, ix);
    if (rc) return rc;
    if ((rc = check_not_mini(ix))) return rc;
    if (ix->rs > 128) return fail(CID_ERR_UNSUPPORTED, "the greedy cover needs at most 8192 colours (index has %u)", ix->n_colors);
    return CID_OK;
}

// The device routine of both entry points.  n > 0 k-mers; d_freq on the device or NULL; fill_rows(d_rows) queues the launches that write
// the n x rs matrix.  Every allocation is made before fill_rows is called: a CID_ERR_NOMEM leaves nothing launched.
template <class FillRows>
int gather_on_device(cid_ctx *c, const cid_index *ix, size_t n, const uint32_t *d_freq, uint64_t min_new, size_t max_rows, FillRows fill_rows,
                     cid_gather_row *out, size_t *n_out, uint64_t *n_hit) {
    const size_t C = ix->n_colors, n_tiles = (n + cid::kWave - 1) / cid::kWave;
    const size_t cap = std::min<size_t>(max_rows, C);   // a colour is emitted at most once
    Scratch s(c);
    uint64_t *d_rows, *d_masks;
    unsigned long long *d_counts;
    cid::GatherRound *d_round;
    cid_gather_row *d_out;
    int rc;
    if ((rc = s.get(n * (size_t)ix->rs, &d_rows)) || (rc = s.get(2 * n_tiles, &d_masks)) || (rc = s.get(3 * C, &d_counts)) || (rc = s.get(1, &d_round)) ||
        (rc = s.get(cap, &d_out)))
        return rc;
    cid::GatherParams p{};
    p.rows = d_rows; p.freq = d_freq; p.n_kmers = n;
    p.rs = ix->rs; p.w64 = ix->w64; p.n_colors = ix->n_colors;
    p.tiles_per_wave = (uint32_t)std::min<size_t>(std::max<size_t>(n_tiles / ((size_t)c->n_cu * 16), 1), 64);
    p.alive = d_masks; p.removed = d_masks + n_tiles;
    p.cnt_new = d_counts; p.total = d_counts + C; p.total_weight = d_counts + 2 * C;
    p.round = d_round; p.out = d_out;
    p.min_new = min_new; p.max_rows = cap;

    if ((rc = fill_rows(d_rows))) return rc;
    cid::GatherRound r{};
    r.live = n;
    HIP_TRY(hipMemcpyAsync(d_round, &r, sizeof(r), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_counts, 0, 3 * C * 8, c->stream));
    HIP_TRY(cid::launch_gather_init(p, c->stream));
    if (cap) {
        HIP_TRY(cid::launch_gather_totals(p, c->stream));
        HIP_TRY(hipMemcpyAsync(p.cnt_new, p.total, C * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(cid::launch_gather_pick(p, c->stream));
    }
    for (;;) {   // one wait a round: has the pick emitted a row?
        HIP_TRY(hipMemcpyAsync(&r, d_round, sizeof(r), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!cap || r.stop) break;
        HIP_TRY(cid::launch_gather_round(p, c->stream));
        HIP_TRY(cid::launch_gather_pick(p, c->stream));
    }
    const size_t rows = std::min<size_t>(r.n_out, cap);
    if (rows) {
        HIP_TRY(hipMemcpyAsync(out, d_out, rows * sizeof(cid_gather_row), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *n_out = rows;
    *n_hit = r.n_hit;
    return CID_OK;
}

}  // namespace

extern "C" {

int cid_search_gather(cid_ctx *c, const cid_index *ix, const uint8_t *kmers, const uint32_t *freq, size_t n_kmers, uint64_t min_new, size_t max_rows,
                      cid_gather_row *out, size_t *n_out, uint64_t *n_hit) {
    int rc = check_gather_args(c, ix, min_new, out, n_out, n_hit);
    if (rc) return rc;
    if (n_kmers && !kmers) return fail(CID_ERR_INVALID, "null argument");
    *n_out = 0; *n_hit = 0;
    if (n_kmers == 0) return CID_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t k = ix->k, chunk = std::min(cid::upload_chunk_kmers(c, k), n_kmers);
    void *d_k;
    if ((rc = slot_reserve(c, S_KMERS, chunk * k, &d_k))) return rc;
    Scratch s(c);
    uint32_t *d_freq = nullptr;
    if (freq && (rc = s.get(n_kmers, &d_freq))) return rc;
    return gather_on_device(c, ix, n_kmers, d_freq, min_new, max_rows, [&](uint64_t *d_rows) -> int {
        if (freq) HIP_TRY(hipMemcpyAsync(d_freq, freq, n_kmers * 4, hipMemcpyHostToDevice, c->stream));
        for (size_t k0 = 0; k0 < n_kmers; k0 += chunk) {   // chunks start on a tile boundary; the stream orders a chunk's upload behind its predecessor's launch
            const size_t nk = std::min(chunk, n_kmers - k0);
            HIP_TRY(hipMemcpyAsync(d_k, kmers + k0 * k, nk * k, hipMemcpyHostToDevice, c->stream));
            const int rc2 = cid::cover_rows_launch(c, ix, cid::DevKeys{(const uint8_t *)d_k, nullptr, nullptr, nk, ix->k, c}, nullptr, d_rows + k0 * ix->rs);
            if (rc2) return rc2;
        }
        return CID_OK;
    }, out, n_out, n_hit);
}

int cid_search_gather_set(cid_ctx *c, const cid_index *ix, const cid_kmerset *ks, uint64_t min_new, size_t max_rows, cid_gather_row *out, size_t *n_out,
                          uint64_t *n_hit) {
    int rc = check_gather_args(c, ix, min_new, out, n_out, n_hit);
    if (rc) return rc;
    cid::DevKeys keys;
    if ((rc = cid::kmerset_keys(ks, &keys))) return rc;
    if (ix->k != keys.k) return fail(CID_ERR_INVALID, "k-mer set k=%u, index k=%u", keys.k, ix->k);
    *n_out = 0; *n_hit = 0;
    if (keys.n == 0) return CID_OK;
    HIP_TRY(hipSetDevice(c->device));
    return gather_on_device(c, ix, keys.n, keys.counts, min_new, max_rows,
                            [&](uint64_t *d_rows) { return cid::cover_rows_launch(c, ix, keys, nullptr, d_rows); }, out, n_out, n_hit);
}

}  // extern "C"
