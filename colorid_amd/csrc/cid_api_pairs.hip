// C ABI of libcolorid_hip.so, part 5: `colorid compare` — the pair counters of an index, shared[i][j] = popcount(column i & column j),
// accumulated from row records or from a resident index.  Kernels: cid_pairs.hip.
#include "cid_api_common.hpp"

using cid::fail;

extern "C" {

int cid_pairs_create(cid_ctx *c, uint64_t bloom_size, uint32_t n_colors, cid_pairs **out) {
    if (!c || !out) return fail(CID_ERR_INVALID, "null ctx/out");
    *out = nullptr;
    if (bloom_size == 0 || n_colors == 0) return fail(CID_ERR_INVALID, "zero parameter");
    if (bloom_size > (1ull << 32)) return fail(CID_ERR_UNSUPPORTED, "bloom_size %llu > 2^32", (unsigned long long)bloom_size);
    if (n_colors > (1u << 20)) return fail(CID_ERR_UNSUPPORTED, "n_colors %u > 2^20", n_colors);
    HIP_TRY(hipSetDevice(c->device));
    const unsigned long long bytes = 8ull * n_colors * n_colors, beside = 256ull << 20;   // the counters, and one upload chunk of records
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b || beside > free_b - bytes)
        return fail(CID_ERR_UNSUPPORTED, "%llu bytes of pair counters for %u colours do not fit beside a 256 MiB chunk of records: %zu bytes of device memory are free",
                    bytes, n_colors, free_b);
    cid_pairs *pr = new (std::nothrow) cid_pairs();
    if (!pr) return fail(CID_ERR_NOMEM, "pairs");
    pr->ctx = c;
    pr->m = bloom_size; pr->n_colors = n_colors; pr->w32 = (n_colors + 31) / 32;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&pr->shared), bytes);
    if (e != hipSuccess) { delete pr; return fail(CID_ERR_NOMEM, "hipMalloc(%llu) for the pair counters: %s", bytes, hipGetErrorString(e)); }
    e = hipMemsetAsync(pr->shared, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(pr->shared); delete pr; return fail(CID_ERR_HIP, "memset: %s", hipGetErrorString(e)); }
    *out = pr;
    return CID_OK;
}

// One call's records through cid::stage_records: each piece is checked on the device (k_pairs_check) before it is counted (k_pairs), so a
// refused piece adds nothing.
int cid_pairs_add_records(cid_pairs *pr, const uint8_t *records, size_t n_records) {
    if (!pr || (n_records && !records)) return fail(CID_ERR_INVALID, "null argument");
    if (n_records == 0) return CID_OK;
    cid_ctx *c = pr->ctx;
    HIP_TRY(hipSetDevice(c->device));
    return cid::stage_records(
        c, records, n_records, pr->w32, 1,
        [&](const uint32_t *d_rec, size_t nr, uint32_t *d_err) {
            return cid::launch_pairs_check(d_rec, pr->w32, nr, pr->m, pr->n_colors, d_err, c->stream);
        },
        [&](const uint32_t *d_rec, size_t nr) {
            cid::PairsParams p{};
            p.rows = d_rec; p.stride = cid::record_words(pr->w32); p.off = cid::kRecordPayload; p.w32 = pr->w32; p.n_rows = nr;
            p.n_colors = pr->n_colors; p.shared = pr->shared;
            HIP_TRY(cid::launch_pairs(p, c->n_cu, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return (int)CID_OK;
        });
}

int cid_pairs_add_index(cid_pairs *pr, const cid_index *ix) {
    if (!pr || !ix) return fail(CID_ERR_INVALID, "null argument");
    if (!ix->finalized) return fail(CID_ERR_INVALID, "index not finalized");
    if (ix->m != pr->m || ix->n_colors != pr->n_colors)
        return fail(CID_ERR_INVALID, "an index of %llu rows x %u colours into pair counters of %llu rows x %u colours", (unsigned long long)ix->m,
                    ix->n_colors, (unsigned long long)pr->m, pr->n_colors);
    cid_ctx *c = pr->ctx;
    if (ix->ctx->device != c->device) return fail(CID_ERR_INVALID, "index lives on device %d, the pair counters on %d", ix->ctx->device, c->device);
    HIP_TRY(hipSetDevice(c->device));
    cid::PairsParams p{};
    p.rows = reinterpret_cast<const uint32_t *>(ix->mat); p.stride = 2ull * ix->rs; p.off = 0; p.w32 = pr->w32; p.n_rows = ix->m;
    p.n_colors = pr->n_colors; p.shared = pr->shared;
    HIP_TRY(cid::launch_pairs(p, c->n_cu, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CID_OK;
}

int cid_pairs_fetch(cid_pairs *pr, uint64_t *shared) {
    if (!pr || !shared) return fail(CID_ERR_INVALID, "null argument");
    cid_ctx *c = pr->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = pr->n_colors;
    HIP_TRY(hipMemcpyAsync(shared, pr->shared, n * n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i)   // the device counts i <= j
        for (size_t j = i + 1; j < n; ++j) shared[j * n + i] = shared[i * n + j];
    return CID_OK;
}

void cid_pairs_destroy(cid_pairs *pr) {
    if (!pr) return;
    (void)hipSetDevice(pr->ctx->device);
    (void)hipStreamSynchronize(pr->ctx->stream);
    if (pr->shared) (void)hipFree(pr->shared);
    delete pr;
}

}  // extern "C"
