// Stand-alone host check of colorid_amd/csrc/host/dists.cpp under ASan + UBSan, no GPU and no libcolorid_hip.so: the table parser, the
// allele encoder (both entrances), the row-block driver, the clustering and the forest and Newick writers, with a plain C++ cid_dists_*
// behind them (the forest: Kruskal over the stand-in's own loop; the neighbour list: the same loop, filtered; the K nearest: the same
// loop, sorted and cut; the histograms: the same loop, counted).
//   make -C tools bin/dists_host_check ;  tools/bin/dists_host_check TABLE PREFIX [T [M [mst [no-matrices]]]] [within=T] [closest=K] [hist]
//   [levels=T1,T2,..] [query=TABLE2]
//   (writes PREFIX.dists.tsv, .compared.tsv, .clusters.tsv; T = - for no clusters; with mst also PREFIX.mst.tsv, .mst.nwk; with within=T
//   also PREFIX.within.tsv; with closest=K also PREFIX.closest.tsv; with hist also PREFIX.hist.tsv; with levels= also PREFIX.levels.tsv
//   (the thresholds as given: put them in descending order); with query=TABLE2 — and within=T or closest=K — PREFIX.query.tsv alone,
//   the two tables aligned by AlleleCodes::from_files)
#include <algorithm>
#include <cstdarg>
#include <numeric>
#include "../colorid_amd/csrc/host/colorid_host.hpp"

namespace colorid {
void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "colorid: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(101);
}
}  // namespace colorid

struct cid_dists { std::vector<uint32_t> codes; uint32_t A, L; };
extern "C" {
const char *cid_last_error(void) { return "stub"; }
int cid_dists_create(cid_ctx *, const uint32_t *codes, uint32_t A, uint32_t L, cid_dists **out) {
    *out = new cid_dists{std::vector<uint32_t>(codes, codes + (size_t)A * L), A, L};
    return 0;
}
int cid_dists_rows(cid_dists *d, uint32_t row0, uint32_t n, uint32_t *differ, uint32_t *compared) {
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t j = 0; j < d->A; ++j) {
            uint32_t c = 0, x = 0;
            for (uint32_t l = 0; l < d->L; ++l) {
                const uint32_t a = d->codes[(size_t)(row0 + r) * d->L + l], b = d->codes[(size_t)j * d->L + l];
                if (a && b) { ++c; x += a != b; }
            }
            differ[(size_t)r * d->A + j] = x;
            if (compared) compared[(size_t)r * d->A + j] = c;
        }
    return 0;
}
// the least edge of every accession into another label, by the loop above
int cid_dists_best(cid_dists *d, const uint32_t *comp, uint32_t min_compared, cid_dists_edge *best) {
    std::vector<uint32_t> differ(d->A), compared(d->A);
    for (uint32_t i = 0; i < d->A; ++i) {
        cid_dists_rows(d, i, 1, differ.data(), compared.data());
        best[i] = cid_dists_edge{i, 0xFFFFFFFFu, 0, 0};
        for (uint32_t j = 0; j < d->A; ++j) {
            if (comp[j] == comp[i] || compared[j] < min_compared) continue;
            if (best[i].b == 0xFFFFFFFFu || differ[j] < best[i].differ || (differ[j] == best[i].differ && compared[j] > best[i].compared))
                best[i] = cid_dists_edge{i, j, differ[j], compared[j]};
        }
    }
    return 0;
}
// Kruskal: every pair with compared >= min_compared, sorted by the edge key
int cid_dists_forest(cid_dists *d, uint32_t min_compared, cid_dists_edge *edges, uint32_t *n_edges, uint32_t *n_rounds) {
    std::vector<cid_dists_edge> all;
    std::vector<uint32_t> differ(d->A), compared(d->A);
    for (uint32_t i = 0; i < d->A; ++i) {
        cid_dists_rows(d, i, 1, differ.data(), compared.data());
        for (uint32_t j = i + 1; j < d->A; ++j)
            if (compared[j] >= min_compared) all.push_back(cid_dists_edge{i, j, differ[j], compared[j]});
    }
    std::sort(all.begin(), all.end(), [](const cid_dists_edge &x, const cid_dists_edge &y) {
        if (x.differ != y.differ) return x.differ < y.differ;
        if (x.compared != y.compared) return x.compared > y.compared;
        return x.a != y.a ? x.a < y.a : x.b < y.b;
    });
    std::vector<uint32_t> parent(d->A);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    *n_edges = 0;
    for (const cid_dists_edge &e : all) {
        const uint32_t a = find(e.a), b = find(e.b);
        if (a == b) continue;
        parent[std::max(a, b)] = std::min(a, b);
        edges[(*n_edges)++] = e;
    }
    *n_rounds = 1;
    return 0;
}
// the pairs of the loop above that pass, in (a, b) order; a small cap makes dists.cpp come back with room
int cid_dists_within(cid_dists *d, uint32_t row0, uint32_t n, uint32_t max_differ, uint32_t min_compared, uint32_t flags, cid_dists_edge *out,
                     size_t cap, uint64_t *n_found) {
    std::vector<uint32_t> differ(d->A), compared(d->A);
    *n_found = 0;
    for (uint32_t i = row0; i < row0 + n; ++i) {
        cid_dists_rows(d, i, 1, differ.data(), compared.data());
        for (uint32_t j = (flags & CID_DISTS_UPPER) ? i + 1 : 0; j < d->A; ++j) {
            if (j == i || compared[j] < min_compared || differ[j] > max_differ) continue;
            if (*n_found < cap) out[*n_found] = cid_dists_edge{i, j, differ[j], compared[j]};
            ++*n_found;
        }
    }
    return 0;
}
// the candidates of the loop above, sorted by (differ, more compared first, b) and cut at k; the ranks past them are "none"
int cid_dists_closest(cid_dists *d, uint32_t row0, uint32_t n, uint32_t k, uint32_t max_differ, uint32_t min_compared, cid_dists_edge *out) {
    std::vector<uint32_t> differ(d->A), compared(d->A);
    std::vector<cid_dists_edge> cand;
    for (uint32_t i = row0; i < row0 + n; ++i) {
        cid_dists_rows(d, i, 1, differ.data(), compared.data());
        cand.clear();
        for (uint32_t j = 0; j < d->A; ++j)
            if (j != i && compared[j] >= min_compared && differ[j] <= max_differ) cand.push_back(cid_dists_edge{i, j, differ[j], compared[j]});
        std::sort(cand.begin(), cand.end(), [](const cid_dists_edge &x, const cid_dists_edge &y) {
            if (x.differ != y.differ) return x.differ < y.differ;
            return x.compared != y.compared ? x.compared > y.compared : x.b < y.b;
        });
        for (uint32_t r = 0; r < k; ++r) out[(size_t)(i - row0) * k + r] = r < cand.size() ? cand[r] : cid_dists_edge{i, 0xFFFFFFFFu, 0, 0};
    }
    return 0;
}
// the pairs of the loop above, counted by compared and — with compared >= min_compared — by differ
int cid_dists_hist(cid_dists *d, uint32_t row0, uint32_t n, uint32_t min_compared, uint32_t flags, uint64_t *differ_hist, uint64_t *compared_hist) {
    std::vector<uint32_t> differ(d->A), compared(d->A);
    std::fill(differ_hist, differ_hist + d->L + 1, (uint64_t)0);
    if (compared_hist) std::fill(compared_hist, compared_hist + d->L + 1, (uint64_t)0);
    for (uint32_t i = row0; i < row0 + n; ++i) {
        cid_dists_rows(d, i, 1, differ.data(), compared.data());
        for (uint32_t j = (flags & CID_DISTS_UPPER) ? i + 1 : 0; j < d->A; ++j) {
            if (j == i) continue;
            if (compared_hist) ++compared_hist[compared[j]];
            if (compared[j] >= min_compared) ++differ_hist[differ[j]];
        }
    }
    return 0;
}
void cid_dists_destroy(cid_dists *d) { delete d; }
}

int main(int argc, char **argv) {
    using namespace colorid;
    DistsOptions o;
    std::string query;
    int kept = 1;   // within=T, closest=K, hist, levels=.. and query=TABLE2 come out of the positional arguments
    for (int i = 1; i < argc; ++i) {
        if (strncmp(argv[i], "within=", 7) == 0) { o.within = true; o.within_threshold = strtoull(argv[i] + 7, nullptr, 10); }
        else if (strncmp(argv[i], "closest=", 8) == 0) o.closest = (uint32_t)strtoul(argv[i] + 8, nullptr, 10);
        else if (strcmp(argv[i], "hist") == 0) o.hist = true;
        else if (strncmp(argv[i], "levels=", 7) == 0)
            for (const char *p = argv[i] + 7; *p;) {
                char *end = nullptr;
                o.levels.push_back(strtoull(p, &end, 10));
                p = *end ? end + 1 : end;
            }
        else if (strncmp(argv[i], "query=", 6) == 0) query = argv[i] + 6;
        else argv[kept++] = argv[i];
    }
    argc = kept;
    if (argc < 3) return 2;
    if (argc > 3 && strcmp(argv[3], "-") != 0) { o.cluster = true; o.threshold = strtoull(argv[3], nullptr, 10); }
    if (argc > 4) o.min_compared = strtoull(argv[4], nullptr, 10);
    o.mst = argc > 5;
    o.no_matrices = argc > 6;
    if (!query.empty()) {
        QueryAlign q;
        const AlleleCodes both = AlleleCodes::from_files(argv[1], query, q);
        dists_query_run(nullptr, both, q, argv[2], o);
        return 0;
    }
    const AlleleCodes t = AlleleCodes::from_file(argv[1]);
    dists_run(nullptr, t, argv[2], o);
    // the in-memory entrance over the same cells
    AlleleTable tab;
    for (size_t a = 0; a < t.accessions.size(); ++a)
        for (size_t l = 0; l < t.loci.size(); ++l)
            if (t.codes[a * t.loci.size() + l]) tab.add(t.loci[l] + "_" + std::to_string(t.codes[a * t.loci.size() + l]), t.accessions[a]);
    const AlleleCodes u = tab.codes(-1);
    fprintf(stderr, "in memory: %zu x %zu\n", u.accessions.size(), u.loci.size());
    return 0;
}
