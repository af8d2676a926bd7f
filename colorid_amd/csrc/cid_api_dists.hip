// C ABI of libcolorid_hip.so, part 6: `colorid dists` — the pairwise allele distances of a cgMLST table: for two accessions the loci both
// have a call at (compared) and those of them where the calls differ (differ).  Kernels: cid_dists.hip.
#include "cid_api_common.hpp"

using cid::fail;

namespace {
void dists_release(cid_dists *d) {
    if (d->codes_t) (void)hipFree(d->codes_t);
    if (d->mask_t) (void)hipFree(d->mask_t);
    delete d;
}
}  // namespace

extern "C" {

// The table goes up in pieces of whole accessions (256 MiB through the ctx's upload slot, at least one accession) and each piece is
// transposed into the resident arrays and checked by the same kernel; the error word is read once, after the last piece, and a refused
// table leaves nothing behind.
int cid_dists_create(cid_ctx *c, const uint32_t *codes, uint32_t n_acc, uint32_t n_loci, cid_dists **out) {
    using namespace cid::slots;
    if (!c || !out) return fail(CID_ERR_INVALID, "null ctx/out");
    *out = nullptr;
    if (!codes) return fail(CID_ERR_INVALID, "null codes");
    if (n_acc == 0 || n_loci == 0) return fail(CID_ERR_INVALID, "zero parameter: %u accessions x %u loci", n_acc, n_loci);
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t Ap = ((uint64_t)n_acc + 63u) & ~63ull;
    const uint32_t W = (uint32_t)(((uint64_t)n_loci + 63u) / 64u);
    if (Ap > (1ull << 60) / n_loci)
        return fail(CID_ERR_UNSUPPORTED, "%u accessions x %u loci: more than 2^62 bytes of allele codes", n_acc, n_loci);
    const unsigned long long row_bytes = 4ull * n_loci;
    const unsigned long long code_bytes = 4ull * n_loci * Ap, mask_bytes = 8ull * W * Ap, block_bytes = 8ull * 64ull * n_acc;
    const unsigned long long piece_rows =   // (launch_dists_put: at most kDistsMaxRowTiles tiles of 64 accessions a piece)
        std::max<unsigned long long>(1, std::min<unsigned long long>({n_acc, (256ull << 20) / row_bytes, 64ull * cid::kDistsMaxRowTiles}));
    const unsigned long long need = code_bytes + mask_bytes + block_bytes + piece_rows * row_bytes;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        return fail(CID_ERR_UNSUPPORTED, "%llu bytes for the allele codes of %u accessions x %u loci, their upload piece and one 64-row block of results do not fit: %zu bytes of device memory are free",
                    need, n_acc, n_loci, free_b);
    cid_dists *d = new (std::nothrow) cid_dists();
    if (!d) return fail(CID_ERR_NOMEM, "dists");
    d->ctx = c;
    d->n_acc = n_acc; d->n_loci = n_loci; d->n_words = W; d->acc_pad = Ap;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d->codes_t), code_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d->mask_t), mask_bytes);
    if (e != hipSuccess) { dists_release(d); return fail(CID_ERR_NOMEM, "hipMalloc(%llu + %llu) for the allele codes: %s", code_bytes, mask_bytes, hipGetErrorString(e)); }
    void *d_piece = nullptr, *d_err = nullptr;
    int rc = cid::slot_reserve(c, S_WORDS, piece_rows * row_bytes, &d_piece);
    if (rc == CID_OK) rc = cid::slot_reserve(c, S_MISC, 16, &d_err);
    if (rc != CID_OK) { dists_release(d); return rc; }
    e = hipMemsetAsync(d->codes_t, 0, code_bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->mask_t, 0, mask_bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, c->stream);
    for (uint64_t a0 = 0; a0 < n_acc && e == hipSuccess; a0 += piece_rows) {
        const uint32_t na = (uint32_t)std::min<uint64_t>(piece_rows, n_acc - a0);
        e = hipMemcpyAsync(d_piece, codes + a0 * n_loci, na * row_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = cid::launch_dists_put((const uint32_t *)d_piece, (uint32_t)a0, na, n_loci, d->codes_t, d->mask_t, Ap, (uint32_t *)d_err, c->stream);
    }
    uint32_t err = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failed launch: nothing of d is in flight when it is freed)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { dists_release(d); return fail(CID_ERR_HIP, "uploading the allele codes: %s", hipGetErrorString(e)); }
    if (err) {
        dists_release(d);
        return fail(CID_ERR_INVALID, "an allele code of 0xFFFFFFFE or 0xFFFFFFFF: codes are 0 (no call) or 1 .. 0xFFFFFFFD");
    }
    *out = d;
    return CID_OK;
}

// The rows go out in slices whose results fit the ctx's dense_report_bytes (at least one row; whole tiles of 64 rows where several fit):
// one launch and one copy per matrix and slice.
int cid_dists_rows(cid_dists *d, uint32_t row0, uint32_t n_rows, uint32_t *differ, uint32_t *compared) {
    if (!d) return fail(CID_ERR_INVALID, "null argument");
    if ((uint64_t)row0 + n_rows > d->n_acc)
        return fail(CID_ERR_INVALID, "rows [%u, %llu) of a table of %u accessions", row0, (unsigned long long)row0 + n_rows, d->n_acc);
    if (n_rows == 0) return CID_OK;
    if (!differ) return fail(CID_ERR_INVALID, "null differ");
    cid_ctx *c = d->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t A = d->n_acc, row_bytes = A * 4;
    uint64_t per = c->tune.dense_report_bytes / (row_bytes * (compared ? 2 : 1));
    per = std::min<uint64_t>(std::max<uint64_t>(per, 1), std::min<uint64_t>(n_rows, 64ull * cid::kDistsMaxRowTiles));
    if (per > 64) per &= ~63ull;
    uint32_t *d_differ = nullptr, *d_compared = nullptr;
    int rc = cid::ctx_alloc(c, per * row_bytes, reinterpret_cast<void **>(&d_differ));
    if (rc != CID_OK) return rc;
    if (compared) {
        rc = cid::ctx_alloc(c, per * row_bytes, reinterpret_cast<void **>(&d_compared));
        if (rc != CID_OK) { cid::ctx_free(c, d_differ); return rc; }
    }
    hipError_t e = hipSuccess;
    for (uint64_t r = 0; r < n_rows && e == hipSuccess; r += per) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(per, n_rows - r);
        cid::DistsParams p{};
        p.T = d->codes_t; p.maskT = d->mask_t; p.Ap = d->acc_pad; p.A = d->n_acc; p.L = d->n_loci; p.W = d->n_words;
        p.row0 = row0 + (uint32_t)r; p.n_rows = n; p.differ = d_differ; p.compared = d_compared;
        e = cid::launch_dists_tile(p, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(differ + r * A, d_differ, n * row_bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && compared) e = hipMemcpyAsync(compared + r * A, d_compared, n * row_bytes, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // the slice's buffers are the next slice's
        if (e == hipSuccess) e = es;
    }
    cid::ctx_free(c, d_differ);
    cid::ctx_free(c, d_compared);
    if (e != hipSuccess) return fail(CID_ERR_HIP, "cid_dists_rows: %s", hipGetErrorString(e));
    return CID_OK;
}

void cid_dists_destroy(cid_dists *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    dists_release(d);
}

}  // extern "C"
