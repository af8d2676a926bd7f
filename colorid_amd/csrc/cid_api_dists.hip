// C ABI of libcolorid_hip.so, part 6: `colorid dists` — the pairwise allele distances of a cgMLST table: for two accessions the loci both
// have a call at (compared) and those of them where the calls differ (differ), and the minimum spanning forest of the accessions under
// them (cid_dists_best, cid_dists_forest), the pairs within a threshold as a list (cid_dists_within), every accession's K nearest
// (cid_dists_closest), and the pairs counted by compared and by differ (cid_dists_hist).  Kernels: cid_dists.hip.
#include "cid_api_common.hpp"

#include <numeric>
#include <vector>

using cid::fail;

namespace {
void dists_release(cid_dists *d) {
    if (d->codes_t) (void)hipFree(d->codes_t);
    if (d->mask_t) (void)hipFree(d->mask_t);
    delete d;
}

// a block of the ctx's cache for the length of a call
template <typename T>
struct Scratch {
    cid_ctx *c;
    T *p = nullptr;
    explicit Scratch(cid_ctx *ctx) : c(ctx) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (p) cid::ctx_free(c, p); }
    int alloc(size_t n) {   // (again: the block before goes back first)
        if (p) cid::ctx_free(c, p);
        p = nullptr;
        return cid::ctx_alloc(c, n * sizeof(T), reinterpret_cast<void **>(&p));
    }
};

constexpr uint32_t kNone = 0xFFFFFFFFu;   // cid_dists_edge.b of an accession without a candidate
static_assert(sizeof(cid_dists_edge) == 16, "cid_dists_edge is part of the ABI");
static_assert(CID_DISTS_CLOSEST_MAX == cid::kDistsClosestMax, "the header's limit is the kernels'");

// the packing limit of k_dists_best's key, refused before anything is launched
int check_best_shape(const cid_dists *d) {
    uint32_t sd, sc;
    if (!cid::dists_best_shifts(d->n_acc, d->n_loci, &sd, &sc))
        return fail(CID_ERR_UNSUPPORTED, "%u accessions x %u loci: 2 ceil(log2(loci + 1)) + ceil(log2 accessions) exceeds the 64 bits of a best-edge key",
                    d->n_acc, d->n_loci);
    return CID_OK;
}

// The device side of one Borůvka round and what stays between rounds: the labels' and the keys' device arrays.
struct BestRound {
    cid_dists *d;
    uint32_t *d_comp = nullptr;
    unsigned long long *d_best = nullptr;
    uint32_t shift_differ = 0, shift_compared = 0;
    explicit BestRound(cid_dists *dd) : d(dd) { (void)cid::dists_best_shifts(d->n_acc, d->n_loci, &shift_differ, &shift_compared); }
    BestRound(const BestRound &) = delete;
    BestRound &operator=(const BestRound &) = delete;
    ~BestRound() {
        if (d_comp) cid::ctx_free(d->ctx, d_comp);
        if (d_best) cid::ctx_free(d->ctx, d_best);
    }
    int run(const uint32_t *comp, uint32_t min_compared, std::vector<unsigned long long> &keys) {
        cid_ctx *c = d->ctx;
        HIP_TRY(hipSetDevice(c->device));
        const size_t A = d->n_acc;
        if (!d_comp) {
            int rc = cid::ctx_alloc(c, A * 4, reinterpret_cast<void **>(&d_comp));
            if (rc == CID_OK) rc = cid::ctx_alloc(c, A * 8, reinterpret_cast<void **>(&d_best));
            if (rc != CID_OK) return rc;
        }
        keys.resize(A);
        cid::DistsParams p{};
        p.T = d->codes_t; p.maskT = d->mask_t; p.Ap = d->acc_pad; p.A = d->n_acc; p.L = d->n_loci; p.W = d->n_words;
        cid::DistsBestParams b{};
        b.comp = d_comp; b.best = d_best; b.min_compared = min_compared;
        hipError_t e = hipMemcpyAsync(d_comp, comp, A * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = cid::launch_dists_best(p, b, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(keys.data(), d_best, A * 8, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failed launch: comp and keys are the caller's)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return fail(CID_ERR_HIP, "cid_dists_best: %s", hipGetErrorString(e));
        return CID_OK;
    }
    cid_dists_edge unpack(uint32_t i, unsigned long long key) const {
        if (key == cid::kDistsNoBest) return cid_dists_edge{i, kNone, 0, 0};
        const unsigned long long low = (1ull << shift_compared) - 1, mid = (1ull << (shift_differ - shift_compared)) - 1;
        const uint32_t compared = d->n_loci - (uint32_t)((key >> shift_compared) & mid);
        return cid_dists_edge{i, (uint32_t)(key & low), (uint32_t)(key >> shift_differ), compared};
    }
};
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

// One round: the labels go up, best[] comes back packed and is unpacked here.  Device memory: 12 bytes an accession.
int cid_dists_best(cid_dists *d, const uint32_t *comp, uint32_t min_compared, cid_dists_edge *best) {
    if (!d || !comp || !best) return fail(CID_ERR_INVALID, "null argument");
    if (min_compared == 0) return fail(CID_ERR_INVALID, "min_compared = 0: two accessions without a common locus are never an edge");
    const int rc = check_best_shape(d);
    if (rc != CID_OK) return rc;
    BestRound round(d);
    std::vector<unsigned long long> keys;
    const int rr = round.run(comp, min_compared, keys);
    if (rr != CID_OK) return rr;
    for (uint32_t i = 0; i < d->n_acc; ++i) best[i] = round.unpack(i, keys[i]);
    return CID_OK;
}

// Borůvka's algorithm with the per-component minimum and the merging on the host: a round is one cid_dists_best with the union-find's
// roots as labels; every component then takes the least (by the edge key) of its members' best edges and is joined along it.  The key is
// a strict total order, so the chosen edges close no cycle and an edge chosen from both ends joins its two components once.  Every round
// that joins anything at least halves the components that still have an edge out, and one more round finds nothing: at most
// floor(log2 A) + 1 rounds.  Device memory: 12 bytes an accession; host memory: 36.
int cid_dists_forest(cid_dists *d, uint32_t min_compared, cid_dists_edge *edges, uint32_t *n_edges, uint32_t *n_rounds) {
    if (!d || !n_edges || !n_rounds) return fail(CID_ERR_INVALID, "null argument");
    *n_edges = *n_rounds = 0;
    if (!edges && d->n_acc > 1) return fail(CID_ERR_INVALID, "null edges");
    if (min_compared == 0) return fail(CID_ERR_INVALID, "min_compared = 0: two accessions without a common locus are never an edge");
    const int rc = check_best_shape(d);
    if (rc != CID_OK) return rc;
    const uint32_t A = d->n_acc;
    if (A == 1) return CID_OK;
    BestRound round(d);
    std::vector<uint32_t> parent(A), comp(A);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    auto less = [](const cid_dists_edge &x, const cid_dists_edge &y) {   // the edge key
        if (x.differ != y.differ) return x.differ < y.differ;
        if (x.compared != y.compared) return x.compared > y.compared;
        if (x.a != y.a) return x.a < y.a;
        return x.b < y.b;
    };
    std::vector<unsigned long long> keys;
    std::vector<cid_dists_edge> pick(A);   // per root the component's least edge of the round (b = none: nothing yet)
    uint32_t n = 0;
    while (n + 1 < A) {
        for (uint32_t i = 0; i < A; ++i) comp[i] = find(i);
        const int rr = round.run(comp.data(), min_compared, keys);
        if (rr != CID_OK) return rr;
        ++*n_rounds;
        for (uint32_t i = 0; i < A; ++i) pick[i].b = kNone;
        bool any = false;
        for (uint32_t i = 0; i < A; ++i) {
            cid_dists_edge e = round.unpack(i, keys[i]);
            if (e.b == kNone) continue;
            if (e.a > e.b) std::swap(e.a, e.b);
            cid_dists_edge &p = pick[comp[i]];
            if (p.b == kNone || less(e, p)) p = e;
            any = true;
        }
        if (!any) break;
        for (uint32_t r = 0; r < A; ++r) {
            if (pick[r].b == kNone) continue;
            const uint32_t x = find(pick[r].a), y = find(pick[r].b);
            if (x == y) continue;   // the other end's component chose the same edge
            parent[std::max(x, y)] = std::min(x, y);
            edges[n++] = pick[r];
        }
    }
    std::sort(edges, edges + n, less);
    *n_edges = n;
    return CID_OK;
}

// The neighbour list.  Device memory: one list of dense_report_bytes / 16 entries (no more than the rows can give, nor than the caller
// has room for) and 8 bytes of cursor, both from the ctx's block cache.  The rows go out in slices of whole 64-row tiles, first as many
// as a launch may hold; after each launch the cursor is read (8 bytes, one stream wait) and says exactly how many entries the slice has.
// They fit the list: that many are copied to out and sorted there by (a, b) — slices are disjoint in a and taken in row order, so the
// whole is sorted.  They do not: a slice of several tiles is halved and both halves run; a slice of one tile runs again with a list
// grown to its count (at most 64 x n_acc entries: the "at least one row a slice" exemption of cid_dists_rows).  Once the caller's cap is
// exceeded nothing more is stored and the remaining slices are only counted (capacity 0: one launch each, never a re-run).
int cid_dists_within(cid_dists *d, uint32_t row0, uint32_t n_rows, uint32_t max_differ, uint32_t min_compared, uint32_t flags,
                     cid_dists_edge *out, size_t cap, uint64_t *n_found) {
    if (!d || !n_found) return fail(CID_ERR_INVALID, "null argument");
    *n_found = 0;
    if (min_compared == 0) return fail(CID_ERR_INVALID, "min_compared = 0: two accessions without a common locus are never within a distance");
    if ((uint64_t)row0 + n_rows > d->n_acc)
        return fail(CID_ERR_INVALID, "rows [%u, %llu) of a table of %u accessions", row0, (unsigned long long)row0 + n_rows, d->n_acc);
    if (flags & ~CID_DISTS_UPPER) return fail(CID_ERR_INVALID, "unknown flags 0x%x", flags & ~CID_DISTS_UPPER);
    if (!out && cap) return fail(CID_ERR_INVALID, "null out with room for %zu entries", cap);
    if (n_rows == 0) return CID_OK;
    cid_ctx *c = d->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t possible = (uint64_t)n_rows * (d->n_acc - 1);
    uint64_t list_cap = std::min<uint64_t>({std::max<uint64_t>(c->tune.dense_report_bytes / sizeof(cid_dists_edge), 1), possible, cap});
    Scratch<uint4> list(c), grown(c);
    Scratch<unsigned long long> cursor(c);
    int rc = cursor.alloc(1);
    if (rc == CID_OK && list_cap) rc = list.alloc(list_cap);
    if (rc != CID_OK) return rc;
    cid::DistsParams p{};
    p.T = d->codes_t; p.maskT = d->mask_t; p.Ap = d->acc_pad; p.A = d->n_acc; p.L = d->n_loci; p.W = d->n_words;
    cid::DistsWithinParams w{};
    w.cursor = cursor.p; w.max_differ = max_differ; w.min_compared = min_compared; w.upper = flags & CID_DISTS_UPPER;
    struct Slice { uint32_t tile0, n_tiles; };   // tiles of 64 rows counted from row0
    const uint32_t tiles = (uint32_t)(((uint64_t)n_rows + 63u) / 64u);
    std::vector<Slice> todo;                      // a stack: the lowest rows on top
    for (uint32_t t0 = tiles; t0 > 0;) {
        const uint32_t n = t0 % cid::kDistsMaxRowTiles ? t0 % cid::kDistsMaxRowTiles : cid::kDistsMaxRowTiles;
        t0 -= n;
        todo.push_back(Slice{t0, n});
    }
    uint64_t total = 0, written = 0;
    bool storing = cap != 0;
    hipError_t e = hipSuccess;
    // one launch: the slice's hits into `into` (room for `room`), *count = how many there are
    auto run = [&](const Slice &s, uint4 *into, uint64_t room, unsigned long long *count) {
        p.row0 = row0 + s.tile0 * 64u;
        p.n_rows = (uint32_t)std::min<uint64_t>((uint64_t)s.n_tiles * 64u, n_rows - (uint64_t)s.tile0 * 64u);
        w.list = into; w.cap = room;
        hipError_t er = hipMemsetAsync(cursor.p, 0, 8, c->stream);
        if (er == hipSuccess) er = cid::launch_dists_within(p, w, c->stream);
        if (er == hipSuccess) er = hipMemcpyAsync(count, cursor.p, 8, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failed launch: count is this frame's)
        return er == hipSuccess ? es : er;
    };
    auto take = [&](const uint4 *from, uint64_t n) {   // a slice's entries: to the caller, sorted
        hipError_t er = hipMemcpyAsync(out + written, from, n * sizeof(cid_dists_edge), hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // the list is the next slice's
        if (er == hipSuccess) er = es;
        if (er != hipSuccess) return er;
        std::sort(out + written, out + written + n, [](const cid_dists_edge &x, const cid_dists_edge &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
        written += n;
        return hipSuccess;
    };
    while (!todo.empty() && e == hipSuccess) {
        const Slice s = todo.back();
        todo.pop_back();
        unsigned long long count = 0;
        e = run(s, storing ? list.p : nullptr, storing ? list_cap : 0, &count);
        if (e != hipSuccess) break;
        if (storing && written + count > cap) storing = false;   // the caller comes back with room: the rest is counted
        if (!storing || count == 0) { total += count; continue; }
        if (count <= list_cap) {
            total += count;
            e = take(list.p, count);
        } else if (s.n_tiles > 1) {
            const uint32_t half = s.n_tiles / 2;
            todo.push_back(Slice{s.tile0 + half, s.n_tiles - half});
            todo.push_back(Slice{s.tile0, half});
        } else {   // one tile of rows and more hits than the list holds: a list of its own, of exactly that many
            rc = grown.alloc(count);
            if (rc != CID_OK) return rc;
            unsigned long long again = 0;
            e = run(s, grown.p, count, &again);
            if (e == hipSuccess && again != count) return fail(CID_ERR_STATE, "cid_dists_within: %llu hits, then %llu, in the same rows", count, again);
            total += count;
            if (e == hipSuccess) e = take(grown.p, count);
        }
    }
    if (e != hipSuccess) return fail(CID_ERR_HIP, "cid_dists_within: %s", hipGetErrorString(e));
    *n_found = total;
    return CID_OK;
}

// The K nearest.  Device memory, all from the ctx's block cache: part, rows x (acc_pad / 64) x k keys of 8 bytes — the rows go out in
// slices of whole 64-row tiles so that it stays within dense_report_bytes, at least one tile a slice whatever the budget (the exemption
// of cid_dists_rows) — and the merge's levels, each a 64th of the one before.  A slice is one k_dists_closest launch, then
// k_dists_closest_merge level by level until a row has one list (one level up to 4 096 accessions, two up to 262 144), then one copy of
// rows x k keys, unpacked here as cid_dists_best's are.  A table of up to 64 accessions has one list a row from the start and still
// takes one level: one path, and the copy reads what the merge wrote.
int cid_dists_closest(cid_dists *d, uint32_t row0, uint32_t n_rows, uint32_t k, uint32_t max_differ, uint32_t min_compared, cid_dists_edge *out) {
    if (!d) return fail(CID_ERR_INVALID, "null argument");
    if (k == 0) return fail(CID_ERR_INVALID, "k = 0: the nearest none");
    if (min_compared == 0) return fail(CID_ERR_INVALID, "min_compared = 0: two accessions without a common locus are never neighbours");
    if ((uint64_t)row0 + n_rows > d->n_acc)
        return fail(CID_ERR_INVALID, "rows [%u, %llu) of a table of %u accessions", row0, (unsigned long long)row0 + n_rows, d->n_acc);
    if (!out && n_rows) return fail(CID_ERR_INVALID, "null out");
    if (k > CID_DISTS_CLOSEST_MAX)
        return fail(CID_ERR_UNSUPPORTED, "k = %u: at most %u nearest an accession (cid_dists_within gives longer lists)", k, CID_DISTS_CLOSEST_MAX);
    int rc = check_best_shape(d);
    if (rc != CID_OK) return rc;
    if (n_rows == 0) return CID_OK;
    cid_ctx *c = d->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t tiles = d->acc_pad / 64u, row_bytes = tiles * k * 8ull;   // of part
    uint64_t per = std::max<uint64_t>(c->tune.dense_report_bytes / row_bytes & ~63ull, 64);
    per = std::min<uint64_t>({per, 64ull * cid::kDistsMaxRowTiles, ((uint64_t)n_rows + 63u) & ~63ull});
    const uint64_t held = std::min<uint64_t>(per, n_rows);   // rows a slice really has
    const uint64_t lists1 = (tiles + 63u) / 64u, lists2 = (lists1 + 63u) / 64u;
    Scratch<unsigned long long> part(c), even(c), odd(c);    // the merge's levels go to even, odd, even, ..
    rc = part.alloc(held * tiles * k);
    if (rc == CID_OK) rc = even.alloc(held * lists1 * k);
    if (rc == CID_OK && lists1 > 1) rc = odd.alloc(held * lists2 * k);
    if (rc != CID_OK) return rc;
    cid::DistsParams p{};
    p.T = d->codes_t; p.maskT = d->mask_t; p.Ap = d->acc_pad; p.A = d->n_acc; p.L = d->n_loci; p.W = d->n_words;
    cid::DistsClosestParams q{};
    q.part = part.p; q.k = k; q.max_differ = max_differ; q.min_compared = min_compared;
    const BestRound key(d);   // (its shifts and its unpack; it allocates nothing until it runs)
    std::vector<unsigned long long> keys(held * k);
    hipError_t e = hipSuccess;
    for (uint64_t r = 0; r < n_rows && e == hipSuccess; r += per) {
        const uint64_t n = std::min<uint64_t>(per, n_rows - r);
        p.row0 = row0 + (uint32_t)r; p.n_rows = (uint32_t)n;
        e = cid::launch_dists_closest(p, q, c->stream);
        const unsigned long long *from = part.p;
        bool to_even = true;
        for (uint64_t lists = tiles; e == hipSuccess;) {
            unsigned long long *to = to_even ? even.p : odd.p;
            e = cid::launch_dists_closest_merge(from, to, n, lists, k, c->stream);
            from = to;
            to_even = !to_even;
            lists = (lists + 63u) / 64u;
            if (lists == 1) break;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(keys.data(), from, n * k * 8ull, hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);   // the slice's buffers are the next slice's
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) break;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t x = 0; x < k; ++x) out[(r + i) * k + x] = key.unpack(row0 + (uint32_t)(r + i), keys[i * k + x]);
    }
    if (e != hipSuccess) return fail(CID_ERR_HIP, "cid_dists_closest: %s", hipGetErrorString(e));
    return CID_OK;
}

// The two histograms.  Device memory: 2 x (n_loci + 1) x 8 bytes from the ctx's block cache, differ's bins and then compared's, set to zero
// on the ctx's stream before the one launch; one copy back and one stream wait.  The rows are not sliced: what comes back does not grow
// with them, and launch_dists_hist takes any number.
int cid_dists_hist(cid_dists *d, uint32_t row0, uint32_t n_rows, uint32_t min_compared, uint32_t flags, uint64_t *differ_hist,
                   uint64_t *compared_hist) {
    if (!d) return fail(CID_ERR_INVALID, "null argument");
    if (!differ_hist) return fail(CID_ERR_INVALID, "null differ_hist");
    if (min_compared == 0) return fail(CID_ERR_INVALID, "min_compared = 0: two accessions without a common locus have no distance to count");
    if ((uint64_t)row0 + n_rows > d->n_acc)
        return fail(CID_ERR_INVALID, "rows [%u, %llu) of a table of %u accessions", row0, (unsigned long long)row0 + n_rows, d->n_acc);
    if (flags & ~CID_DISTS_UPPER) return fail(CID_ERR_INVALID, "unknown flags 0x%x", flags & ~CID_DISTS_UPPER);
    const size_t bins = (size_t)d->n_loci + 1;
    std::fill(differ_hist, differ_hist + bins, (uint64_t)0);
    if (compared_hist) std::fill(compared_hist, compared_hist + bins, (uint64_t)0);
    if (n_rows == 0) return CID_OK;
    cid_ctx *c = d->ctx;
    HIP_TRY(hipSetDevice(c->device));
    Scratch<unsigned long long> dev(c);
    const int rc = dev.alloc(2 * bins);
    if (rc != CID_OK) return rc;
    cid::DistsParams p{};
    p.T = d->codes_t; p.maskT = d->mask_t; p.Ap = d->acc_pad; p.A = d->n_acc; p.L = d->n_loci; p.W = d->n_words;
    p.row0 = row0; p.n_rows = n_rows;
    cid::DistsHistParams h{};
    h.differ_hist = dev.p; h.compared_hist = dev.p + bins; h.min_compared = min_compared; h.upper = flags & CID_DISTS_UPPER;
    std::vector<unsigned long long> back((compared_hist ? 2 : 1) * bins);
    hipError_t e = hipMemsetAsync(dev.p, 0, 2 * bins * 8, c->stream);
    if (e == hipSuccess) e = cid::launch_dists_hist(p, h, c->n_cu, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back.data(), dev.p, back.size() * 8, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failed launch: back is this frame's)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(CID_ERR_HIP, "cid_dists_hist: %s", hipGetErrorString(e));
    std::copy(back.begin(), back.begin() + (ptrdiff_t)bins, differ_hist);
    if (compared_hist) std::copy(back.begin() + (ptrdiff_t)bins, back.end(), compared_hist);
    return CID_OK;
}

void cid_dists_destroy(cid_dists *d) {
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    dists_release(d);
}

}  // extern "C"
