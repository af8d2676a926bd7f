// Shared by the translation units behind the C ABI (cid_api_ctx / _index / _search / _readid / _pairs / _dists .hip); not part of the ABI.
// stage_records: the one path of .bxi row records (cid_records.hpp) from a caller's memory to the kernels of load, merge, subset and compare.
#pragma once
#include "../../include/colorid_hip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "cid_host_math.hpp"
#include "cid_internal.hpp"
#include "cid_objects.hpp"
#include "cid_records.hpp"

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return cid::fail(CID_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace cid {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Work per block: enough blocks to balance 256 CUs dynamically, few enough that the per-block flush of the
// LDS counters (<= 3*C global atomics) stays negligible.
inline uint32_t pick_tiles_per_block(const cid_ctx *c, uint64_t n_kmers) {
    const uint64_t n_tiles = (n_kmers + kWave - 1) / kWave;
    uint64_t tpb = n_tiles / ((uint64_t)c->n_cu * 32);
    if (tpb < 4) tpb = 4;
    if (tpb > 256) tpb = 256;
    return (uint32_t)tpb;
}

// k-mers per chunk of the pipelined host-pointer calls (cid_ctx_tune "upload_chunk_bytes" / CID_UPLOAD_CHUNK_BYTES: 256 MiB at k + 8 bytes
// a k-mer).  Chunks start on a tile boundary: 64*k bytes keep the 16-byte alignment of the k-mer array; a budget below k + 8 bytes
// (0 included) still moves a tile per chunk
inline size_t upload_chunk_kmers(const cid_ctx *c, size_t k) {
    const size_t chunk = ((size_t)c->tune.upload_chunk_bytes / (k + 8) + 63) & ~(size_t)63;
    return chunk ? chunk : 64;
}

// check_record's bits as the error of the call
inline int fail_malformed_records(uint32_t err) {
    return fail(CID_ERR_INVALID, "malformed row record(s):%s%s%s%s", (err & 1) ? " word count != ceil(n_colors/32)" : "",
                (err & 2) ? " bit count != n_colors" : "", (err & 4) ? " row >= bloom_size" : "", (err & 8) ? " bits beyond n_colors" : "");
}

// One call's row records (of a file whose rows have w32_rec words) through the ctx's upload slots, piece by piece: S_WORDS takes the
// records, S_MISC the error word; launch(d_records, n, d_err) starts the kernel that checks them (check_record -> d_err) and returns its
// hipError_t; the piece's error word is read back and refused here; then(d_records, n) runs after a clean check and returns a CID code.
// The stream is idle when a piece is done: the slot is the next piece's (and the next call's) upload buffer.
// A piece is 256 MiB of records, and no more than 2^30 threads a launch at threads_per_record threads each.  A record has at most
// 24 + 4 * 32768 bytes, so a piece never comes to zero records; a launch with no more threads per record than the record has words
// (plain put, subset, compare's check) never reaches the thread cap — only merge's plan can.
template <class Launch, class Then>
int stage_records(cid_ctx *c, const uint8_t *records, size_t n_records, uint32_t w32_rec, uint64_t threads_per_record, Launch launch, Then then) {
    using namespace slots;
    const size_t rec_bytes = 4 * record_words(w32_rec);
    const size_t batch = std::max<size_t>(1, std::min<size_t>((256u << 20) / rec_bytes, (1ull << 30) / threads_per_record));
    for (size_t r0 = 0; r0 < n_records; r0 += batch) {
        const size_t nr = std::min(n_records - r0, batch);
        void *d_rec, *d_err;
        int rc = slot_reserve(c, S_WORDS, nr * rec_bytes, &d_rec);
        if (rc) return rc;
        rc = slot_reserve(c, S_MISC, 16, &d_err);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_err, 0, 4, c->stream));
        HIP_TRY(hipMemcpyAsync(d_rec, records + r0 * rec_bytes, nr * rec_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch((const uint32_t *)d_rec, nr, (uint32_t *)d_err));
        uint32_t err = 0;
        HIP_TRY(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (err) return fail_malformed_records(err);
        rc = then((const uint32_t *)d_rec, nr);
        if (rc) return rc;
    }
    return CID_OK;
}
template <class Launch>
int stage_records(cid_ctx *c, const uint8_t *records, size_t n_records, uint32_t w32_rec, uint64_t threads_per_record, Launch launch) {
    return stage_records(c, records, n_records, w32_rec, threads_per_record, launch, [](const uint32_t *, size_t) { return (int)CID_OK; });
}

}  // namespace cid
