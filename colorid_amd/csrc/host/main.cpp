// `colorid` command line: the reference's drop-in surface for the query path (src/main.rs) —
//   search  (src/main.rs:127-217, :555-628)   read_id (:241-328, :704-868)   batch_id (:329-418, :869-888: read_id over a sample sheet)
//   build   (:31-126, :466-554; needed to produce .bxi files)   info (:218-240, :630-703)
// Same flag letters, defaults, stdout/stderr/file formats.  Extra flags: --device N, --gpus N | --devices a,b,.. (search, read_id:
// the query is sharded over the GPUs), --hash xxh3_v08|xxh3_v07.  Extra commands:
// hashcheck (which hash variant was an index built with); merge (indices of one shape and disjoint accessions as one index, the
// file `build` writes over the union of their reference lists); subset (chosen accessions of an index as an index of their own, the
// file `build` writes over the kept lines of the reference list); compare (all-pairs similarity of an index's accessions: which of
// them are duplicates — the question before `subset -x`); fold (an index at a smaller Bloom size that divides its own, the file
// `build -s` writes at that size: an over-sized index shrunk, or two indices brought to one size before `merge`); collapse (several
// accessions of an index as one colour, the rows `build` writes over the members' sequences joined: strain-level index -> taxon-level);
// alleles (the accessions x loci table of a cgMLST scheme from saved `search -s -m` rows; `search -s -m --alleles` makes it in the run);
// dists (pairwise allele distances and single-linkage clusters of such a table; `search -s -m --alleles PREFIX --dists` makes them in the run).
// Minimizer indices (.mxi): build -m [-v M], info, read_id, batch_id.  Not provided (outside the query path): read_filter.
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <unistd.h>

#include "colorid_host.hpp"

using namespace colorid;

namespace {

// Which way a run leaves is decided once, here, and `colorid --help` says how:
//   COLORID_FAST_EXIT=1      always the short way;  COLORID_FAST_EXIT=0 or COLORID_FULL_TEARDOWN=1: always the orderly way;
//   neither set              the short way unless something in the process may still have output to write at exit: a preloaded library
//                            (LD_PRELOAD, /etc/ld.so.preload), a profiler's tool library (rocprofv3 writes its files from an exit handler),
//                            coverage counters (LLVM_PROFILE_FILE, GCOV_PREFIX).
// Either way every output file is closed and stdout / stderr are flushed — and checked — before (leave()).
const char *g_exit_reason = "nothing in the process writes at exit";
bool tool_may_write_at_exit() {
    for (const char *v : {"LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_LIBRARY_CTOR", "HSA_TOOLS_LIB", "LLVM_PROFILE_FILE", "GCOV_PREFIX"})
        if (const char *e = getenv(v)) if (*e) { g_exit_reason = v; return true; }   // (not a switch: other tools' variables that announce something writing at exit)
    if (FILE *f = fopen("/etc/ld.so.preload", "r")) {
        int ch;
        bool any = false;
        while ((ch = fgetc(f)) != EOF) if (!isspace(ch)) { any = true; break; }
        fclose(f);
        if (any) { g_exit_reason = "/etc/ld.so.preload"; return true; }
    }
    return false;
}
bool decide_orderly_exit() {
    if (const char *e = cli_env("COLORID_FAST_EXIT")) { g_exit_reason = "COLORID_FAST_EXIT"; return atoi(e) == 0; }
    if (cli_env("COLORID_FULL_TEARDOWN")) { g_exit_reason = "COLORID_FULL_TEARDOWN"; return true; }
    return tool_may_write_at_exit();
}
bool g_orderly_exit = decide_orderly_exit();


struct Args {
    std::map<std::string, std::vector<std::string>> values;  // canonical long name -> values
    std::map<std::string, bool> flags;
    bool has(const std::string &k) const { return values.count(k) && !values.at(k).empty(); }
    const std::string &one(const std::string &k) const { return values.at(k)[0]; }
};

struct OptSpec { char shrt; const char *lng; bool takes_value; bool multi; };

Args parse(int argc, char **argv, int first, const std::vector<OptSpec> &spec) {
    Args a;
    for (int i = first; i < argc; ++i) {
        std::string tok = argv[i];
        const OptSpec *o = nullptr;
        if (tok.size() > 2 && tok[0] == '-' && tok[1] == '-') {
            for (auto &s : spec) if (tok.substr(2) == s.lng) o = &s;
        } else if (tok.size() == 2 && tok[0] == '-') {
            for (auto &s : spec) if (s.shrt == tok[1]) o = &s;
        }
        if (!o) die("error: Found argument '%s' which wasn't expected, or isn't valid in this context", tok.c_str());
        if (!o->takes_value) { a.flags[o->lng] = true; continue; }
        if (i + 1 >= argc) die("error: The argument '--%s' requires a value but none was supplied", o->lng);
        a.values[o->lng].push_back(argv[++i]);
        while (o->multi && i + 1 < argc && argv[i + 1][0] != '-') a.values[o->lng].push_back(argv[++i]);
    }
    return a;
}

template <typename T>
T num_or(const Args &a, const char *k, T dflt) {  // value_t!(..).unwrap_or(dflt): a value that does not parse gives the default
    if (!a.has(k)) return dflt;
    char *end = nullptr;
    const std::string &s = a.one(k);
    if constexpr (std::is_floating_point<T>::value) {
        const double v = strtod(s.c_str(), &end);
        return (end && *end == 0 && !s.empty()) ? (T)v : dflt;
    } else {
        const long long v = strtoll(s.c_str(), &end, 10);
        return (end && *end == 0 && !s.empty()) ? (T)v : dflt;
    }
}

bool ends_with(const std::string &s, const char *suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// --gpus N (devices 0..N-1) or --devices a,b,... (an id may repeat: several ranks on one GPU): reads / k-mers are sharded over
// the ranks, the index is replicated, per-accession counters are all-reduced (RCCL over xGMI).  The reference's -t (rayon threads,
// src/main.rs:718-721) has no meaning here and is ignored with a note.
// --placement striped (with --gpus / --devices): the INDEX is sharded instead — rank r holds a stripe of colours of every row, every
// rank sees the whole query (an index larger than one GPU's HBM).
struct Gpus {
    cid_group *group = nullptr;            // nullptr: one GPU (--device)
    cid_ctx *ctx = nullptr;                // rank 0's context (or the only one)
    std::vector<cid_index *> replicas;     // replicas, or the stripes
    bool striped = false;
};

std::vector<int> device_list(const Args &a) {
    std::vector<int> ids;
    if (a.has("devices")) {
        const std::string &s = a.one("devices");
        size_t p = 0;
        while (p <= s.size()) {
            const size_t e = s.find(',', p);
            const std::string tok = s.substr(p, e == std::string::npos ? std::string::npos : e - p);
            char *end = nullptr;
            const long v = strtol(tok.c_str(), &end, 10);
            if (tok.empty() || *end) die("--devices expects a comma-separated list of device ids, got '%s'", s.c_str());
            ids.push_back((int)v);
            if (e == std::string::npos) break;
            p = e + 1;
        }
    } else if (a.has("gpus")) {
        const int n = num_or<int>(a, "gpus", 1);
        if (n < 1) die("--gpus expects a positive number");
        for (int i = 0; i < n; ++i) ids.push_back(i);
    }
    return ids;
}

// COLORID_TIMING=1: wall-clock milliseconds of the CLI's phases on stderr
const bool g_timing = cli_env("COLORID_TIMING") != nullptr;
const auto g_t_start = std::chrono::steady_clock::now();
void phase_done(const char *what) {
    if (!g_timing) return;
    static auto last = g_t_start;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "timing: %s %.0f ms (at %.0f ms)\n", what, std::chrono::duration<double, std::milli>(now - last).count(),
            std::chrono::duration<double, std::milli>(now - g_t_start).count());
    last = now;
}

// RCCL prints its version banner (and whatever NCCL_DEBUG asks for) to the C stdout while communicators are made and destroyed; a
// drop-in `colorid search` prints result rows only.  The library never touches a file descriptor, so the CLI does it here, around
// those two calls and nowhere near the searches: while an object of this class lives, fd 1 is fd 2.  (Nothing else of this process
// writes to stdout at those two moments: the banner row is printed before, the result rows between them.)
class StdoutToStderr {
  public:
    StdoutToStderr() {
        fflush(stdout);
        saved_ = dup(1);
        if (saved_ >= 0) dup2(2, 1);
    }
    ~StdoutToStderr() {
        fflush(stdout);
        if (saved_ >= 0) { dup2(saved_, 1); close(saved_); }
    }
  private:
    int saved_;
};

Gpus make_gpus(const Args &a) {
    Gpus g;
    if (a.has("bigsi")) bigsi_read_ahead(a.one("bigsi"));   // the index file's pages come in beside the runtime's start-up
    if (a.has("threads"))
        fprintf(stderr, "note: -t %s is ignored: the search runs on the GPU (--gpus N shards the query over N GPUs)\n", a.one("threads").c_str());
    const std::vector<int> ids = device_list(a);
    if (a.has("placement")) {
        const std::string &pl = a.one("placement");
        if (pl == "striped") g.striped = true;
        else if (pl != "replicated") die("--placement expects replicated or striped, got '%s'", pl.c_str());
    }
    const bool one_rank_group = ids.size() == 1 && (cli_env("COLORID_REDUCE") || g.striped);   // the group path with a single rank
    if (ids.size() <= 1 && !one_rank_group) {
        if (g.striped) die("--placement striped needs --gpus N or --devices a,b,...");
        const int dev = ids.empty() ? num_or<int>(a, "device", 0) : ids[0];
        if (cid_ctx_create(dev, &g.ctx) != CID_OK) die("cannot open GPU %d: %s (colorid has no CPU search path)", dev, cid_last_error());
        return g;
    }
    {
        StdoutToStderr quiet;
        if (cid_group_create(ids.data(), (int)ids.size(), &g.group) != CID_OK) die("cannot open %zu GPUs: %s", ids.size(), cid_last_error());
        g_orderly_exit = true;   // (RCCL communicators are alive from here on: such a run always leaves through release())
    }
    if (cid_group_ctx(g.group, 0, &g.ctx) != CID_OK) die("%s", cid_last_error());
    int rccl = 0;
    cid_group_uses_rccl(g.group, &rccl);
    if (g.striped)
        fprintf(stderr, "%zu ranks, one colour stripe of the index each; per-k-mer facts are summed %s\n", ids.size(),
                rccl ? "with RCCL all-reduce" : "with peer copies");
    else
        fprintf(stderr, "%zu ranks; per-accession counters are reduced %s\n", ids.size(), rccl ? "with RCCL all-reduce" : "through the host");
    return g;
}

// The device code of the kernels a command will launch is loaded on a helper thread while the index loads (cid_warmup): the
// runtime would otherwise load it inside the first search / read_id call (~60 ms for the read_id kernels).  The helper thread is on the
// critical path when the index is small (a 1.7 GB index loads in 42 ms, the read_id units in 64-94): nothing goes in that does not pay for
// itself — not CID_WARM_COLD (40 ms for a path few inputs take), not CID_WARM_PIPES (the index upload has woken the bus and the queues);
// round 6 measured both: profiles/r06_warm_ab.txt.
std::thread warm_async(const Gpus &g, unsigned what) {
    std::vector<cid_ctx *> ctxs;
    if (g.group) {
        int n = 0;
        cid_group_size(g.group, &n);
        for (int r = 0; r < n; ++r) { cid_ctx *c = nullptr; if (cid_group_ctx(g.group, r, &c) == CID_OK) ctxs.push_back(c); }
    } else ctxs.push_back(g.ctx);
    if (const char *e = cli_env("COLORID_WARM")) what = (unsigned)strtoul(e, nullptr, 0);   // (A/B runs: another mask, 0 = nothing ahead of its first use)
    return std::thread([ctxs, what] { for (cid_ctx *c : ctxs) (void)cid_warmup(c, what); });   // (a failure here shows up in the first real call)
}

void replicate(Gpus &g, Bigsi &b) {   // after the index is loaded on rank 0
    if (!g.group) return;
    if (g.striped) { set_stripes(g.group, g.replicas); return; }   // load_index put the stripes in place
    int n = 0;
    cid_group_size(g.group, &n);
    g.replicas.assign((size_t)n, nullptr);
    if (cid_group_replicate_index(g.group, b.index, g.replicas.data()) != CID_OK) die("replicating the index: %s", cid_last_error());
    set_group(g.group, g.replicas);
}

// The process is about to end and its results are written and closed: freeing gigabytes of HBM object by object, unloading the code
// objects and the runtime's own teardown buy nothing — the driver reclaims a process's memory in one go — but cost 0.1-0.2 s of a
// 0.7 s `read_id`.  One-GPU runs therefore skip release() and leave through leave(); COLORID_FULL_TEARDOWN=1 (the sanitizer runs,
// anybody embedding the drivers) keeps the orderly way, and so do multi-GPU runs (RCCL communicators are shut down properly).

void release(Gpus &g, Bigsi &b) {
    if (!g_orderly_exit && !g.group) { cid_ctx_synchronize(g.ctx); return; }
    g_orderly_exit = true;
    for (cid_index *ix : g.replicas)
        if (ix && ix != b.index) cid_index_destroy(ix);
    if (b.index) cid_index_destroy(b.index);
    if (g.group) { StdoutToStderr quiet; cid_group_destroy(g.group); }   // owns the contexts
    else cid_ctx_destroy(g.ctx);
}

cid_ctx *make_ctx(const Args &a) {
    cid_ctx *ctx = nullptr;
    if (a.has("threads"))
        fprintf(stderr, "note: -t %s is ignored: k-mer counting and Bloom inserts run on the GPU\n", a.one("threads").c_str());
    const int dev = num_or<int>(a, "device", 0);
    if (cid_ctx_create(dev, &ctx) != CID_OK) die("cannot open GPU %d: %s (colorid has no CPU search path)", dev, cid_last_error());
    return ctx;
}

const char *const kHashNames[CID_HASH_VARIANTS] = {"xxh3_v08", "xxh3_v07"};

int hash_variant(const Args &a) {
    if (!a.has("hash")) return CID_HASH_XXH3_V08;
    for (int v = 0; v < CID_HASH_VARIANTS; ++v)
        if (a.one("hash") == kHashNames[v]) return v;
    die("unknown --hash '%s' (available: xxh3_v08, xxh3_v07)", a.one("hash").c_str());
}

Bigsi load_index(cid_ctx *ctx, const Args &a, bool meta_only = false, Gpus *gpus = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "Loading index\n");
    // The file format carries no hash id and the reference's hash crate (xxh3 ^0.1.1) cannot be run here: an index written by
    // this program matches its own --hash; for one written by the Rust binary, `colorid hashcheck` decides which --hash applies.
    if (!meta_only && !a.has("hash") && !cli_env("COLORID_QUIET"))
        fprintf(stderr, "note: --hash defaults to xxh3_v08 (published XXH3); parity with an index built by the Rust colorid is unverified — "
                        "run `colorid hashcheck -b <index> -r <ref_file>` once to find the variant it was built with\n");
    const bool striped = gpus && gpus->striped;
    Bigsi b = read_bigsi(ctx, a.one("bigsi"), hash_variant(a), meta_only, striped ? gpus->group : nullptr, striped ? &gpus->replicas : nullptr);
    fprintf(stderr, "Index loaded in %ld seconds\n",
            (long)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count());
    return b;
}

const std::vector<OptSpec> kCommon = {{0, "device", true, false}, {0, "hash", true, false}, {0, "gpus", true, false}, {0, "devices", true, false},
                                      {0, "placement", true, false}};

std::vector<OptSpec> with_common(std::vector<OptSpec> v) {
    v.insert(v.end(), kCommon.begin(), kCommon.end());
    return v;
}

int cmd_build(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'r', "refs", true, false}, {'k', "kmer", true, false},
                                                     {'n', "num_hashes", true, false}, {'s', "bloom", true, false}, {'m', "minimizer", false, false},
                                                     {'v', "value", true, false}, {'t', "threads", true, false}, {'Q', "quality", true, false},
                                                     {'f', "filter", true, false}}));
    for (const char *req : {"bigsi", "refs", "kmer", "num_hashes", "bloom"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    printf(" Ref_file : %s\n Bigsi file : %s\nK-mer size: %s\nBloom filter parameters: num hashes %s, filter size %s\n",
           a.one("refs").c_str(), a.one("bigsi").c_str(), a.one("kmer").c_str(), a.one("num_hashes").c_str(), a.one("bloom").c_str());
    const bool minimizer = a.flags.count("minimizer") > 0;
    uint64_t m_value = 0;
    if (minimizer) {   // main.rs:480-486; -v defaults to 15 and must parse (the reference unwraps)
        const std::string v = a.has("value") ? a.one("value") : std::string("15");
        char *end = nullptr;
        m_value = strtoull(v.c_str(), &end, 10);
        if (v.empty() || *end) die("called `Result::unwrap()` on an `Err` value: ParseIntError (-v %s)", v.c_str());
        printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)m_value);
    }
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    Bigsi b = build_single(ctx, a.one("refs"), num_or<uint64_t>(a, "bloom", 50000000), num_or<uint64_t>(a, "num_hashes", 4),
                           num_or<uint64_t>(a, "kmer", 31), num_or<uint8_t>(a, "quality", 15), num_or<int64_t>(a, "filter", -1),
                           hash_variant(a), m_value);
    phase_done("accessions counted and inserted");
    printf("Saving BIGSI to file.\n");
    save_bigsi(a.one("bigsi") + (minimizer ? ".mxi" : ".bxi"), b);
    phase_done("index written");
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return 0;
}

// merge: -b OUT -i a.bxi b.bxi [...] writes OUT.bxi (OUT.mxi for .mxi inputs): every accession of every input, colours in name order,
// rows and n_ref_kmers as `build` over the union of the reference lists writes them.  Everything that would refuse the merge is checked
// on the inputs' headers before the GPU is opened; the rows then go to the device one upload chunk at a time (the inputs are never
// held there whole).  The file format carries no hash id: the inputs must have been built with one hash variant (`colorid hashcheck`).
int cmd_merge(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'b', "bigsi", true, false}, {'i', "input", true, true}, {0, "device", true, false}});
    for (const char *req : {"bigsi", "input"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const std::vector<std::string> &paths = a.values.at("input");
    const bool minimizer = ends_with(paths[0], ".mxi");
    const std::string out = a.one("bigsi") + (minimizer ? ".mxi" : ".bxi");
    std::vector<MergeInput> inputs;
    Bigsi b = merge_check(paths, out, inputs);
    phase_done("inputs checked");
    std::string in_list, parts;
    for (const MergeInput &in : inputs) {
        in_list += (in_list.empty() ? "" : " ") + in.path;
        parts += (parts.empty() ? "" : " + ") + std::to_string(in.meta.colors.size());
    }
    printf(" Input indices : %s\n Bigsi file : %s\nK-mer size: %llu\nBloom filter parameters: num hashes %llu, filter size %llu\n", in_list.c_str(),
           out.c_str(), (unsigned long long)b.k_size, (unsigned long long)b.num_hash, (unsigned long long)b.bloom_size);
    if (minimizer) printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)b.m_size);
    printf("Accessions: %zu (%s)\n", b.colors.size(), parts.c_str());
    for (const MergeInput &in : inputs) bigsi_read_ahead(in.path);   // pages come in beside the runtime's start-up, as for `search`
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    merge_records(ctx, b, inputs);
    phase_done("records streamed and deposited");
    if (cid_index_finalize(b.index) != CID_OK) die("cid_index_finalize: %s", cid_last_error());
    phase_done("finalize");
    printf("Saving BIGSI to file.\n");
    save_bigsi(out, b);
    phase_done("index written");
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return 0;
}

// subset: -b OUT -i in.bxi (-a keep.txt | -x drop.txt) writes OUT.bxi (OUT.mxi for an .mxi input): the listed accessions (-x: all the
// others), colours renumbered in their order, rows and n_ref_kmers as `build` over the kept lines of the reference list writes them.
// Everything that would refuse it is checked on the header, the n_ref_kmers tail and the list before the GPU is opened; the rows then go
// to the device one upload chunk at a time: the device holds the output index, never the input's matrix.
int cmd_subset(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'b', "bigsi", true, false}, {'i', "input", true, true}, {'a', "accessions", true, false},
                                         {'x', "exclude", true, false}, {0, "device", true, false}});
    for (const char *req : {"bigsi", "input"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    if (a.has("accessions") == a.has("exclude"))
        die("subset needs exactly one of -a/--accessions (the accessions to keep) and -x/--exclude (the accessions to drop), got %s",
            a.has("accessions") ? "both" : "neither");
    for (const char *k : {"accessions", "exclude"})
        if (a.has(k) && a.values.at(k).size() != 1) die("subset takes one list file, got %zu for --%s", a.values.at(k).size(), k);
    const std::vector<std::string> &paths = a.values.at("input");
    if (paths.size() != 1) die("subset takes exactly one input index (-i in.bxi), got %zu: %s ...", paths.size(), paths[1].c_str());
    const bool exclude = a.has("exclude");
    const std::string &list = a.one(exclude ? "exclude" : "accessions");
    const bool minimizer = ends_with(paths[0], ".mxi");
    const std::string out = a.one("bigsi") + (minimizer ? ".mxi" : ".bxi");
    SubsetInput in;
    Bigsi b = subset_check(paths[0], out, list, exclude, in);
    phase_done("input checked");
    printf(" Input index : %s\n Bigsi file : %s\nK-mer size: %llu\nBloom filter parameters: num hashes %llu, filter size %llu\n", in.path.c_str(),
           out.c_str(), (unsigned long long)b.k_size, (unsigned long long)b.num_hash, (unsigned long long)b.bloom_size);
    if (minimizer) printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)b.m_size);
    printf("Accessions: %zu of %zu kept\n", b.colors.size(), in.meta.colors.size());
    bigsi_read_ahead(in.path);   // pages come in beside the runtime's start-up, as for `search`
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    subset_records(ctx, b, in);
    phase_done("records streamed and extracted");
    if (cid_index_finalize(b.index) != CID_OK) die("cid_index_finalize: %s", cid_last_error());
    phase_done("finalize");
    printf("Saving BIGSI to file.\n");
    save_bigsi(out, b);
    phase_done("index written");
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return 0;
}

// fold: -b OUT -i in.bxi (-s NEW_BLOOM_SIZE | -f FACTOR | -p MAX_FALSE_POSITIVE) writes OUT.bxi (OUT.mxi for an .mxi input): the index
// `build -s NEW_BLOOM_SIZE` writes over the same reference list — same header but for the size, same colours, same n_ref_kmers — made
// from the index alone: NEW_BLOOM_SIZE must divide the input's size (-f F: the input's size / F; -p P: the smallest divisor at which no
// accession's predicted false-positive rate, as `info` prints it, exceeds P).  Everything that would refuse it is checked on the header
// and the n_ref_kmers tail before the GPU is opened; the rows then go to the device one upload chunk at a time: the device holds the
// output index, never the input's matrix.
int cmd_fold(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'b', "bigsi", true, false}, {'i', "input", true, true}, {'s', "bloom", true, false},
                                         {'f', "factor", true, false}, {'p', "max_false_positive", true, false}, {0, "device", true, false}});
    for (const char *req : {"bigsi", "input"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const struct { char by; const char *key; } ways[] = {{'s', "bloom"}, {'f', "factor"}, {'p', "max_false_positive"}};
    std::string given;
    char by = 0;
    const char *key = nullptr;
    for (const auto &w : ways)
        if (a.has(w.key)) {
            given += std::string(given.empty() ? "-" : ", -") + w.by;
            by = w.by;
            key = w.key;
            if (a.values.at(w.key).size() != 1) die("fold takes one value for -%c/--%s, got %zu", w.by, w.key, a.values.at(w.key).size());
        }
    if (given.size() != 2)
        die("fold needs exactly one of -s/--bloom (the new Bloom size), -f/--factor (the divisor of the size) and -p/--max_false_positive "
            "(the highest predicted false-positive rate of any accession), got %s", given.empty() ? "none" : given.c_str());
    const std::vector<std::string> &paths = a.values.at("input");
    if (paths.size() != 1) die("fold takes exactly one input index (-i in.bxi), got %zu: %s ...", paths.size(), paths[1].c_str());
    const bool minimizer = ends_with(paths[0], ".mxi");
    const std::string out = a.one("bigsi") + (minimizer ? ".mxi" : ".bxi");
    FoldInput in;
    Bigsi b = fold_check(paths[0], out, by, a.one(key), in);
    phase_done("input checked");
    printf(" Input index : %s\n Bigsi file : %s\nK-mer size: %llu\nBloom filter parameters: num hashes %llu, filter size %llu\n", in.path.c_str(),
           out.c_str(), (unsigned long long)b.k_size, (unsigned long long)b.num_hash, (unsigned long long)b.bloom_size);
    if (minimizer) printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)b.m_size);
    printf("Filter size: %llu of %llu (factor %llu)\n", (unsigned long long)b.bloom_size, (unsigned long long)in.meta.bloom_size,
           (unsigned long long)in.factor);
    if (by == 'p')
        printf("False positive bound %s: accession %s predicts %.6g at filter size %llu, the highest of %zu\n", a.one(key).c_str(),
               b.colors[in.worst].c_str(), in.worst_fp, (unsigned long long)b.bloom_size, b.colors.size());
    fflush(stdout);              // the choice is on record whatever becomes of the GPU
    bigsi_read_ahead(in.path);   // pages come in beside the runtime's start-up, as for `search`
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    fold_records(ctx, b, in);
    phase_done("records streamed and folded");
    if (cid_index_finalize(b.index) != CID_OK) die("cid_index_finalize: %s", cid_last_error());
    phase_done("finalize");
    printf("Saving BIGSI to file.\n");
    save_bigsi(out, b);
    phase_done("index written");
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return 0;
}

// compare: -i idx.bxi|idx.mxi -o PREFIX [-t MIN_JACCARD] [-d DUP_JACCARD]: every accession's Bloom filter against every other's, from the
// index alone.  shared[i][j] = popcount(column i & column j) is counted on the GPU (cid_pairs_*) while the records stream through it one
// upload chunk at a time; the reports follow from it in double arithmetic.  With a = bits[i], b = bits[j], s = shared[i][j], u = a + b - s:
//   PREFIX_accessions.tsv  accession, n_ref_kmers, bits, fill = bits/M, fp_stated = false_prob(M, N, n_ref_kmers) (as `info`), fp_measured = fill^N
//   PREFIX_pairs.tsv       a, b, shared, jaccard_bits = s/u, jaccard_kmers — every i < j with jaccard_bits >= -t (default 0: all), by (i, j).
//                          jaccard_kmers takes the Bloom cardinality estimate card(x) = -(M/N) ln(1 - x/M): max(0, card(a) + card(b) - card(u)) / card(u)
//                          (0 when card(u) = 0; `nan` when u = M, a saturated union)
//   PREFIX_duplicates.txt  (-d T) colour j is a duplicate when an earlier colour that is not itself one has jaccard_bits >= T: a `subset -x` list
// Everything that would refuse it is checked on the header and the n_ref_kmers tail before the GPU is opened, but counters that do not fit.
namespace {
double compare_threshold(const Args &a, const char *key, char letter, double dflt) {
    if (!a.has(key)) return dflt;
    const std::string &s = a.one(key);
    char *end = nullptr;
    const double v = strtod(s.c_str(), &end);
    if (s.empty() || *end || !(v >= 0.0 && v <= 1.0)) die("compare: -%c/--%s expects a number in [0, 1], got '%s'", letter, key, s.c_str());
    return v;
}
FILE *compare_out(const std::string &path) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("compare: could not create %s", path.c_str());
    setvbuf(f, nullptr, _IOFBF, 1u << 20);
    return f;
}
void compare_close(FILE *f, const std::string &path) {
    if (fclose(f) != 0) die("compare: writing %s failed", path.c_str());
}
}  // namespace

int cmd_compare(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'i', "input", true, true}, {'o', "output", true, false}, {'t', "min_jaccard", true, false},
                                         {'d', "duplicates", true, false}, {0, "device", true, false}});
    for (const char *req : {"input", "output"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const std::vector<std::string> &paths = a.values.at("input");
    if (paths.size() != 1) die("compare takes exactly one input index (-i idx.bxi), got %zu: %s ...", paths.size(), paths[1].c_str());
    const double min_jaccard = compare_threshold(a, "min_jaccard", 't', 0.0);
    const bool want_dups = a.has("duplicates");
    const double dup_jaccard = compare_threshold(a, "duplicates", 'd', 1.0);
    const std::string &prefix = a.one("output");
    CompareInput in;
    compare_check(paths[0], in);
    phase_done("input checked");
    const Bigsi &b = in.meta;
    printf(" Input index : %s\nK-mer size: %llu\nBloom filter parameters: num hashes %llu, filter size %llu\n", in.path.c_str(),
           (unsigned long long)b.k_size, (unsigned long long)b.num_hash, (unsigned long long)b.bloom_size);
    if (b.m_size) printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)b.m_size);
    const size_t nc = b.colors.size();
    printf("Accessions: %zu, rows: %llu\n", nc, (unsigned long long)in.n_rows);
    bigsi_read_ahead(in.path);   // pages come in beside the runtime's start-up, as for `search`
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    const std::vector<uint64_t> shared = compare_records(ctx, in);
    phase_done("records streamed and counted");
    const double M = (double)b.bloom_size, N = (double)b.num_hash;
    auto jaccard_bits = [&](size_t i, size_t j) {
        const double s = (double)shared[i * nc + j], u = (double)shared[i * nc + i] + (double)shared[j * nc + j] - s;
        return u == 0.0 ? 0.0 : s / u;
    };
    auto card = [&](double x) { return -(M / N) * std::log(1.0 - x / M); };
    {
        const std::string path = prefix + "_accessions.tsv";
        FILE *f = compare_out(path);
        fprintf(f, "accession\tn_ref_kmers\tbits\tfill\tfp_stated\tfp_measured\n");
        for (size_t c = 0; c < nc; ++c) {
            const double fill = (double)shared[c * nc + c] / M;
            fprintf(f, "%s\t%llu\t%llu\t%.6f\t%.6f\t%.6f\n", b.colors[c].c_str(), (unsigned long long)b.n_ref_kmers[c],
                    (unsigned long long)shared[c * nc + c], fill, false_prob(M, N, (double)b.n_ref_kmers[c]), std::pow(fill, N));
        }
        compare_close(f, path);
    }
    uint64_t reported = 0;
    {
        const std::string path = prefix + "_pairs.tsv";
        FILE *f = compare_out(path);
        fprintf(f, "a\tb\tshared\tjaccard_bits\tjaccard_kmers\n");
        for (size_t i = 0; i < nc; ++i)
            for (size_t j = i + 1; j < nc; ++j) {
                const double jb = jaccard_bits(i, j);
                if (!(jb >= min_jaccard)) continue;
                const double x = (double)shared[i * nc + i], y = (double)shared[j * nc + j], s = (double)shared[i * nc + j], u = x + y - s;
                ++reported;
                if (u == M) {   // a saturated union: its cardinality estimate is infinite
                    fprintf(f, "%s\t%s\t%llu\t%.6f\tnan\n", b.colors[i].c_str(), b.colors[j].c_str(), (unsigned long long)shared[i * nc + j], jb);
                    continue;
                }
                const double cu = card(u);
                const double jk = cu == 0.0 ? 0.0 : std::max(0.0, card(x) + card(y) - cu) / cu;
                fprintf(f, "%s\t%s\t%llu\t%.6f\t%.6f\n", b.colors[i].c_str(), b.colors[j].c_str(), (unsigned long long)shared[i * nc + j], jb, jk);
            }
        compare_close(f, path);
    }
    printf("Pairs reported: %llu of %llu\n", (unsigned long long)reported, (unsigned long long)((uint64_t)nc * (nc - 1) / 2));
    if (want_dups) {
        std::vector<char> dup(nc, 0);
        size_t n_dup = 0;
        const std::string path = prefix + "_duplicates.txt";
        FILE *f = compare_out(path);
        for (size_t j = 0; j < nc; ++j) {
            for (size_t i = 0; i < j && !dup[j]; ++i)
                if (!dup[i] && jaccard_bits(i, j) >= dup_jaccard) dup[j] = 1;
            if (dup[j]) { ++n_dup; fprintf(f, "%s\n", b.colors[j].c_str()); }
        }
        compare_close(f, path);
        printf("Duplicates: %zu of %zu accessions\n", n_dup, nc);
    }
    phase_done("reports written");
    cid_ctx_destroy(ctx);
    return 0;
}

// collapse: -b OUT -i in.bxi -g GROUPS.tsv writes OUT.bxi (OUT.mxi for an .mxi input): one colour per group of accessions, row r colour g
// the OR of row r over the members of g — the row records `build` writes over a reference list with one line per group whose FASTA is
// the members' FASTA files joined; colours in byte order of the group names, same Bloom size, hashes, k and minimizer size.  GROUPS.tsv:
// `accession TAB group` per line; an unlisted accession stays a group of its own, a listed one alone in its group is renamed.  The
// union's k-mer count is not in the index: n_ref_kmers of a group of several is estimated from fill (collapse_n_ref).  OUT_groups.tsv
// reports per output colour: group, members, n_ref_kmers, n_ref_sum (the members' counts added), bits, fill = bits/M, fp_stated =
// false_prob(M, N, n_ref_kmers) (as `info`), fp_measured = fill^N — collapsing raises fill; `fold -p` is the tool that sizes an index by
// that bound.  Everything that would refuse it is checked on the header, the n_ref_kmers tail and the groups file before the GPU is
// opened; the rows then go to the device one upload chunk at a time: the device holds the output index, never the input's matrix.
int cmd_collapse(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'i', "input", true, true}, {'g', "groups", true, false}}));
    for (const char *req : {"bigsi", "input", "groups"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    for (const char *k : {"gpus", "devices", "placement"})
        if (a.has(k)) die("collapse runs on one GPU (--device D): --%s is not provided", k);
    if (a.values.at("groups").size() != 1) die("collapse takes one groups file, got %zu for --groups", a.values.at("groups").size());
    const std::vector<std::string> &paths = a.values.at("input");
    if (paths.size() != 1) die("collapse takes exactly one input index (-i in.bxi), got %zu: %s ...", paths.size(), paths[1].c_str());
    const bool minimizer = ends_with(paths[0], ".mxi");
    const std::string out = a.one("bigsi") + (minimizer ? ".mxi" : ".bxi"), report = a.one("bigsi") + "_groups.tsv";
    CollapseInput in;
    Bigsi b = collapse_check(paths[0], out, a.one("groups"), in);
    phase_done("input checked");
    printf(" Input index : %s\n Bigsi file : %s\nK-mer size: %llu\nBloom filter parameters: num hashes %llu, filter size %llu\n", in.path.c_str(),
           out.c_str(), (unsigned long long)b.k_size, (unsigned long long)b.num_hash, (unsigned long long)b.bloom_size);
    if (minimizer) printf("Build with minimizers, minimizer size: %llu\n", (unsigned long long)b.m_size);
    printf("Accessions: %zu in %zu groups\n", in.meta.colors.size(), b.colors.size());
    bigsi_read_ahead(in.path);   // pages come in beside the runtime's start-up, as for `search`
    cid_ctx *ctx = make_ctx(a);
    phase_done("GPU context");
    collapse_records(ctx, b, in);
    phase_done("records streamed and collapsed");
    if (cid_index_finalize(b.index) != CID_OK) die("cid_index_finalize: %s", cid_last_error());
    phase_done("finalize");
    printf("Saving BIGSI to file.\n");
    save_bigsi(out, b);
    phase_done("index written");
    {
        FILE *f = compare_out(report);
        const double M = (double)b.bloom_size, N = (double)b.num_hash;
        fprintf(f, "group\tmembers\tn_ref_kmers\tn_ref_sum\tbits\tfill\tfp_stated\tfp_measured\n");
        for (size_t g = 0; g < b.colors.size(); ++g) {
            std::string members;
            uint64_t sum = 0;
            for (const uint32_t c : in.members[g]) {
                members += (members.empty() ? "" : ",") + in.meta.colors[c];
                sum += in.meta.n_ref_kmers[c];
            }
            const double fill = (double)in.bits_index[g] / M;
            fprintf(f, "%s\t%s\t%llu\t%llu\t%llu\t%.6f\t%.6f\t%.6f\n", b.colors[g].c_str(), members.c_str(), (unsigned long long)b.n_ref_kmers[g],
                    (unsigned long long)sum, (unsigned long long)in.bits_index[g], fill, false_prob(M, N, (double)b.n_ref_kmers[g]), std::pow(fill, N));
        }
        compare_close(f, report);
    }
    phase_done("report written");
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return 0;
}

// --max-missing N (search --alleles, alleles): -1 when absent
long long max_missing_arg(const Args &a) {
    if (!a.has("max-missing")) return -1;
    const std::string &v = a.one("max-missing");
    char *end = nullptr;
    const long long n = strtoll(v.c_str(), &end, 10);
    if (v.empty() || *end || n < 0) die("error: --max-missing expects a number of cells (0 or more), got '%s'", v.c_str());
    return n;
}

// --cluster T / --within T / --min-compared M (search --dists, dists): a number of loci
uint64_t loci_arg(const Args &a, const char *key) {
    const std::string &v = a.one(key);
    char *end = nullptr;
    errno = 0;
    const long long n = strtoll(v.c_str(), &end, 10);
    if (v.empty() || *end || n < 0 || errno) die("error: --%s expects a number of loci (0 or more), got '%s'", key, v.c_str());
    return (uint64_t)n;
}
// --closest K (search --dists, dists): a number of neighbours, 1 .. CID_DISTS_CLOSEST_MAX
uint32_t closest_arg(const Args &a) {
    const std::string &v = a.one("closest");
    char *end = nullptr;
    errno = 0;
    const long long n = strtoll(v.c_str(), &end, 10);
    if (v.empty() || *end || errno || n < 1 || n > (long long)CID_DISTS_CLOSEST_MAX)
        die("error: --closest expects a number of neighbours from 1 to %u, got '%s' (--within T lists every accession within a distance, however many)",
            CID_DISTS_CLOSEST_MAX, v.c_str());
    return (uint32_t)n;
}
// --levels T1,T2,.. (search --dists, dists): 1 .. kDistsMaxLevels different numbers of loci, in any order; returned coarse to fine
std::vector<uint64_t> levels_arg(const Args &a) {
    const std::string &v = a.values.at("levels")[0];
    std::vector<uint64_t> levels;
    bool ok = !v.empty();
    for (size_t at = 0; ok && at <= v.size();) {
        const size_t comma = std::min(v.find(',', at), v.size());
        const std::string item = v.substr(at, comma - at);
        char *end = nullptr;
        errno = 0;
        const unsigned long long n = strtoull(item.c_str(), &end, 10);
        ok = !item.empty() && item.find_first_not_of("0123456789") == std::string::npos && !*end && !errno &&
             std::find(levels.begin(), levels.end(), (uint64_t)n) == levels.end() && levels.size() < kDistsMaxLevels;
        levels.push_back((uint64_t)n);
        at = comma + 1;
    }
    if (!ok)
        die("error: --levels expects 1 to %zu different numbers of loci (0 or more) separated by commas, as in 0,2,7, got '%s'", kDistsMaxLevels,
            v.c_str());
    std::sort(levels.begin(), levels.end(), std::greater<uint64_t>());
    return levels;
}
// what --cluster, --within, --closest, --hist, --levels, --min-compared, --mst and --no-matrices ask for; refuses --min-compared without
// --cluster, --mst, --within, --closest, --hist or --levels, and --no-matrices when nothing else would be written
DistsOptions dists_options(const Args &a) {
    DistsOptions o;
    o.mst = a.flags.count("mst") != 0;
    o.no_matrices = a.flags.count("no-matrices") != 0;
    o.hist = a.flags.count("hist") != 0;
    const bool levels = a.values.count("levels") != 0;   // (an empty list is refused as a list, not overlooked)
    if (a.has("min-compared") && !a.has("cluster") && !o.mst && !a.has("within") && !a.has("closest") && !o.hist && !levels)
        die("error: --min-compared needs --cluster T (it is the least number of loci two accessions must share to be linked), --mst or --within T, or --closest K, "
            "--hist or --levels T1,T2,..");
    if (o.no_matrices && !a.has("cluster") && !o.mst && !a.has("within") && !a.has("closest") && !o.hist && !levels)
        die("error: --no-matrices needs --mst or --cluster T or --within T (without the two matrices nothing would be written), or --closest K, --hist or "
            "--levels T1,T2,..");
    if (levels) o.levels = levels_arg(a);
    if (a.has("closest")) o.closest = closest_arg(a);
    if (a.has("cluster")) { o.cluster = true; o.threshold = loci_arg(a, "cluster"); }
    if (a.has("within")) { o.within = true; o.within_threshold = loci_arg(a, "within"); }
    if (a.has("min-compared")) o.min_compared = loci_arg(a, "min-compared");
    return o;
}

// what --gather-min and --gather-max carry: a count of at least 1
uint64_t gather_arg(const Args &a, const char *key) {
    const std::string v = a.one(key);
    char *end = nullptr;
    errno = 0;
    const unsigned long long n = strtoull(v.c_str(), &end, 10);
    if (v.empty() || v[0] == '-' || *end || errno || n == 0) die("error: --%s expects a number of 1 or more, got '%s'", key, v.c_str());
    return (uint64_t)n;
}

int cmd_search(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'q', "query", true, true}, {'r', "reverse", true, true},
                                                     {'f', "filter", true, false}, {'p', "p_shared", true, false}, {'g', "gene_search", false, false},
                                                     {'s', "perfect_search", false, false}, {'m', "multi_fasta", false, false},
                                                     {'Q', "quality", true, false}, {0, "coverage", false, false},
                                                     {0, "alleles", true, false}, {0, "max-missing", true, false},
                                                     {0, "nearest", false, false}, {0, "dists", false, false},
                                                     {0, "cluster", true, false}, {0, "min-compared", true, false},
                                                     {0, "mst", false, false}, {0, "no-matrices", false, false}, {0, "within", true, false},
                                                     {0, "closest", true, false}, {0, "hist", false, false}, {0, "levels", true, false},
                                                     {0, "gather", true, false}, {0, "gather-min", true, false}, {0, "gather-max", true, false}}));
    for (const char *req : {"bigsi", "query"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const std::vector<std::string> files1 = a.values.at("query");
    // --gather PREFIX [--gather-min N] [--gather-max R]: after each query's search, the greedy cover of its k-mers by accessions
    // (cid_search_gather) into PREFIX.gather.tsv.  The query's whole k-mer map against a whole index on one GPU; everything else is
    // refused here, before the GPU context is made
    batch_search_pe::GatherOut gather;
    if (a.has("gather")) {
        const std::pair<const char *, const char *> other[] = {{"gene_search", "-g"}, {"perfect_search", "-s"}, {"multi_fasta", "-m"}, {"coverage", "--coverage"}};
        for (const auto &o : other)
            if (a.flags.count(o.first)) die("error: --gather reads a whole query's k-mers against the index and does not go with %s", o.second);
        for (const char *opt : {"gpus", "devices", "placement"})
            if (a.has(opt)) die("error: --gather runs on one GPU: it does not go with --%s", opt);
        if (cli_env("COLORID_REDUCE")) die("error: --gather runs on one GPU: it does not go with COLORID_REDUCE");
    } else {
        for (const char *opt : {"gather-min", "gather-max"})
            if (a.has(opt)) die("error: --%s needs --gather PREFIX (it bounds the rows of PREFIX.gather.tsv)", opt);
    }
    if (a.has("gather-min")) gather.min_new = gather_arg(a, "gather-min");
    if (a.has("gather-max")) gather.max_rows = (size_t)gather_arg(a, "gather-max");
    // -s -m --alleles PREFIX [--max-missing N]: the rows of -s -m, and the accessions x loci table made from them (AlleleTable) once
    // the last file is done.  What does not go together is refused here, before the GPU context is made
    if (a.has("alleles")) {
        if (a.flags.count("gene_search")) die("error: --alleles makes the allele table of a perfect search (-s -m) and does not go with -g");
        if (!a.flags.count("perfect_search") || !a.flags.count("multi_fasta"))
            die("error: --alleles needs -s -m (every FASTA record an allele, perfect search)");
    } else if (a.has("max-missing")) {
        die("error: --max-missing needs --alleles PREFIX (it chooses which accessions go to PREFIX.clean.tsv)");
    }
    const long long max_missing = max_missing_arg(a);
    // -s -m --alleles PREFIX --nearest [-p MIN_SHARE]: for the cells the tables cannot call, the closest allele (PREFIX.nearest.tsv, from
    // cid_search_nearest_segments on every batch).  The per-record route of groups and colour stripes has no counters: refused here,
    // before the GPU context is made
    const bool nearest = a.flags.count("nearest") != 0;
    if (nearest) {
        if (!a.has("alleles")) die("error: --nearest needs -s -m --alleles PREFIX (it writes PREFIX.nearest.tsv beside the allele tables)");
        if (a.has("gpus") || a.has("devices") || a.has("placement") || cli_env("COLORID_REDUCE"))
            die("error: --nearest runs on one GPU: it does not go with --gpus, --devices, --placement or COLORID_REDUCE");
    }
    // -s -m --alleles PREFIX --dists [--cluster T] [--within T] [--closest K] [--hist] [--levels T1,T2,..] [--mst] [--min-compared M]
    // [--no-matrices]: after the tables, the pairwise allele distances of the raw table's accessions (the clean table's with
    // --max-missing), the pairs within T, every accession's K nearest, the pairs counted by distance, their clusters at one threshold
    // or several and their minimum spanning forest, on this run's context: the files `colorid dists -t PREFIX.raw.tsv` writes.  Refused here, before the GPU context is made
    const bool dists = a.flags.count("dists") != 0;
    if (dists && !a.has("alleles")) die("error: --dists needs -s -m --alleles PREFIX (it writes PREFIX.dists.tsv from the allele table)");
    if (!dists && a.has("cluster")) die("error: --cluster needs --dists (it clusters the allele distances)");
    if (!dists && a.has("within")) die("error: --within needs --dists (it lists the pairs of accessions at most T alleles apart)");
    if (!dists && a.has("closest")) die("error: --closest needs --dists (it lists every accession's K nearest by allele distance)");
    if (!dists && a.flags.count("mst")) die("error: --mst needs --dists (it is the minimum spanning forest of the allele distances)");
    if (!dists && a.flags.count("hist")) die("error: --hist needs --dists (it counts the pairs of accessions by their allele distance)");
    if (!dists && a.values.count("levels")) die("error: --levels needs --dists (it clusters the allele distances at several thresholds)");
    if (!dists && a.flags.count("no-matrices")) die("error: --no-matrices needs --dists (it leaves out PREFIX.dists.tsv and PREFIX.compared.tsv)");
    const DistsOptions dists_opt = dists_options(a);
    // -g -m --coverage: where on each record an accession hits (cid_search_cover).  FASTA records on one GPU; everything else is refused
    // here, before the GPU context is made
    const bool coverage = a.flags.count("coverage") != 0;
    if (coverage) {
        if (!a.flags.count("gene_search") || !a.flags.count("multi_fasta") || a.flags.count("perfect_search"))
            die("error: --coverage needs -g -m (every FASTA record its own query) and does not go with -s");
        for (const std::string &f : files1)
            if (ends_with(f, "gz")) die("error: --coverage takes FASTA queries, not reads: %s", f.c_str());
        if (a.has("gpus") || a.has("devices") || a.has("placement"))
            die("error: --coverage runs on one GPU: it does not go with --gpus, --devices or --placement");
    }
    const std::vector<std::string> files2 = a.has("reverse") && a.one("reverse") != "none" ? a.values.at("reverse") : std::vector<std::string>{};
    const int64_t filter = num_or<int64_t>(a, "filter", -1);
    const double cov = num_or<double>(a, "p_shared", 0.35);
    const uint8_t quality = num_or<uint8_t>(a, "quality", 15);
    if (ends_with(a.one("bigsi"), ".mxi")) {
        fprintf(stderr, "Error: An index with minimizers (.mxi) is used, but not available for this function\n");
        return 0;
    }
    if (cli_env("COLORID_GPU_INFLATE") && atoi(cli_env("COLORID_GPU_INFLATE")) > 0) LineReader::inflate_on_gpu(num_or<int>(a, "device", 0));
    // gzip decoding of the first query starts now and runs beside GPU start-up and the index load; a block-gzip query on one GPU goes
    // up compressed instead (cid_fastq_count_kmers: its members are read ahead, the k-mer map is counted from text that never leaves HBM)
    unsigned warm_what = CID_WARM_SEARCH;
    if (!a.flags.count("perfect_search") && ends_with(files1[0], "gz")) {
        std::vector<std::string> fq{files1[0]};
        if (!files2.empty()) fq.push_back(files2[0]);
        const bool one_gpu = !a.has("gpus") && !a.has("devices") && !a.has("placement") && !cli_env("COLORID_REDUCE");
        const bool host_kmers = cli_env("COLORID_HOST_KMERS") != nullptr;
        if (one_gpu && !host_kmers && read_id_mt_pe::device_fastq_wanted(fq, fq.size())) {
            warm_what |= CID_WARM_INFLATE | CID_WARM_FASTQ;
            for (const std::string &f : fq)
                BgzfMemberReader::prefetch(f, read_id_mt_pe::device_fastq_stretch_bytes(0), read_id_mt_pe::device_fastq_host_share(),
                                           read_id_mt_pe::device_fastq_host_threads(fq.size()));
        } else {
            for (const std::string &f : fq) LineReader::prefetch(f);
        }
    }
    Gpus gpus = make_gpus(a);
    phase_done("GPU context");
    std::thread warm = warm_async(gpus, warm_what);
    cid_ctx *ctx = gpus.ctx;
    Bigsi b = load_index(ctx, a, false, &gpus);
    replicate(gpus, b);
    warm.join();
    phase_done("index load");
    if (coverage) {
        if (b.colors.size() > 8192)
            die("error: --coverage serves indices of at most 8192 accessions; %s has %zu", a.one("bigsi").c_str(), b.colors.size());
        batch_search_pe::batch_search_cover(ctx, files1, b, cov);
    } else if (a.flags.count("perfect_search")) {
        if (a.flags.count("multi_fasta")) {
            if (nearest && b.colors.size() > 8192)
                die("error: --nearest serves indices of at most 8192 accessions; %s has %zu", a.one("bigsi").c_str(), b.colors.size());
            AlleleTable table;
            const std::unique_ptr<NearestTable> near(nearest ? new NearestTable(b.colors.size()) : nullptr);
            perfect_search::batch_search_mf(ctx, files1, b, a.has("alleles") ? &table : nullptr, near.get());
            if (a.has("alleles")) { fflush(stdout); table.write(a.one("alleles"), max_missing); }
            const double min_share = cov;   // -p: for --nearest the least share of a record's k-mers that is worth a line
            if (near) near->write(a.one("alleles"), b.colors, min_share);
            if (dists) dists_run(ctx, table.codes(max_missing), a.one("alleles"), dists_opt);
        } else perfect_search::batch_search(ctx, files1, b);
    } else if (a.flags.count("gene_search") && a.flags.count("multi_fasta") &&
               std::none_of(files1.begin(), files1.end(), [](const std::string &f) { return ends_with(f, "gz"); })) {
        batch_search_pe::batch_search_mf(ctx, files1, b, cov);   // -g -m: every FASTA record is its own query
    } else if (a.has("gather")) {
        if (b.m_size) die("error: --gather does not serve an index with minimizers: %s", a.one("bigsi").c_str());
        if (b.colors.size() > 8192)
            die("error: --gather serves indices of at most 8192 accessions; %s has %zu", a.one("bigsi").c_str(), b.colors.size());
        gather.open(a.one("gather"));
        batch_search_pe::batch_search(ctx, files1, files2, b, filter, cov, false, quality, &gather);
        gather.finish();
    } else {
        batch_search_pe::batch_search(ctx, files1, files2, b, filter, cov, a.flags.count("gene_search") > 0, quality);
    }
    phase_done("search");
    LineReader::drop_prefetched();
    BgzfMemberReader::drop_prefetched();
    release(gpus, b);
    phase_done("release");
    return 0;
}

// alleles: -r ROWS -o PREFIX [--max-missing N] — the table writer of `search -s -m --alleles` over rows saved earlier (the stdout of a
// `search -s -m` run: lines of fewer than four TAB-separated fields, the banner and the warnings, are skipped).  No GPU is opened.
int cmd_alleles(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'r', "rows", true, false}, {'o', "output", true, false}, {0, "max-missing", true, false}});
    for (const char *req : {"rows", "output"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const long long max_missing = max_missing_arg(a);
    AlleleTable table;
    table.add_rows_file(a.one("rows"));
    table.write(a.one("output"), max_missing);
    return 0;
}

// dists: -t TABLE -o PREFIX [--cluster T] [--within T] [--closest K] [--mst] [--min-compared M] [--no-matrices] — PREFIX.dists.tsv and
// PREFIX.compared.tsv (and PREFIX.clusters.tsv; PREFIX.within.tsv; PREFIX.closest.tsv; PREFIX.mst.tsv and PREFIX.mst.nwk) from a table in the form of
// PREFIX.raw.tsv / PREFIX.clean.tsv.  The flags are checked before the table is read, the table is read and checked before the GPU is
// opened; a table without accessions or without loci needs none.
// dists: -t TABLE --query TABLE2 -o PREFIX --within T [--min-compared M] — PREFIX.query.tsv alone: the neighbours of TABLE2's accessions
// among TABLE's and each other, the loci matched by name; a query table without accessions needs no GPU.
// --closest K (1 .. 64, checked with the flags): every accession's K nearest — PREFIX.closest.tsv, within T where --within is given too —
// and with --query, where it may stand in for --within, the first K lines of every query accession's list.
// --hist: PREFIX.hist.tsv, the unordered pairs counted by differ and by compared; --levels T1,T2,.. (1 .. 32 of them, checked with the
// flags): PREFIX.levels.tsv, every accession's cluster at each threshold.  Neither goes with --query.
int cmd_dists(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'t', "table", true, false}, {'o', "output", true, false}, {0, "cluster", true, false},
                                         {0, "min-compared", true, false}, {0, "mst", false, false}, {0, "no-matrices", false, false},
                                         {0, "within", true, false}, {0, "closest", true, false}, {0, "query", true, false},
                                         {0, "hist", false, false}, {0, "levels", true, false}, {0, "device", true, false}});
    for (const char *req : {"table", "output"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    if (a.has("query")) {
        if (!a.has("within") && !a.has("closest"))
            die("error: --query needs --within T or --closest K (it lists the query accessions' neighbours at most T alleles apart, or the K nearest of each)");
        if (a.has("cluster")) die("error: --query writes PREFIX.query.tsv alone and does not go with --cluster");
        if (a.flags.count("mst")) die("error: --query writes PREFIX.query.tsv alone and does not go with --mst");
        if (a.flags.count("no-matrices")) die("error: --query writes PREFIX.query.tsv alone and does not go with --no-matrices (no matrix is made)");
        if (a.flags.count("hist")) die("error: --query writes PREFIX.query.tsv alone and does not go with --hist");
        if (a.values.count("levels")) die("error: --query writes PREFIX.query.tsv alone and does not go with --levels");
    }
    const DistsOptions opt = dists_options(a);
    if (a.has("query")) {
        QueryAlign q;
        const AlleleCodes both = AlleleCodes::from_files(a.one("table"), a.one("query"), q);
        phase_done("tables read");
        cid_ctx *ctx = nullptr;
        if (both.accessions.size() > q.n_table && !both.loci.empty()) {
            ctx = make_ctx(a);
            phase_done("GPU context");
        }
        dists_query_run(ctx, both, q, a.one("output"), opt, phase_done);
        if (ctx) cid_ctx_destroy(ctx);
        return 0;
    }
    const AlleleCodes table = AlleleCodes::from_file(a.one("table"));
    phase_done("table read");
    cid_ctx *ctx = nullptr;
    if (!table.accessions.empty() && !table.loci.empty()) {
        ctx = make_ctx(a);
        phase_done("GPU context");
    }
    dists_run(ctx, table, a.one("output"), opt, phase_done);
    if (ctx) cid_ctx_destroy(ctx);
    return 0;
}

int cmd_info(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'c', "compressed", true, false}}));
    if (!a.has("bigsi")) die("error: The following required arguments were not provided: --bigsi");
    Bigsi b = load_index(nullptr, a, /*meta_only=*/true);
    if (b.m_size)   // main.rs:645-648
        printf("BIGSI parameters:\nBloomfilter-size: %llu\nNumber of hashes: %llu\nK-mer size: %llu\n minimizer size: %llu\n\n",
               (unsigned long long)b.bloom_size, (unsigned long long)b.num_hash, (unsigned long long)b.k_size, (unsigned long long)b.m_size);
    else
        printf("BIGSI parameters:\nBloomfilter-size: %llu\nNumber of hashes: %llu\nK-mer size: %llu\n", (unsigned long long)b.bloom_size,
               (unsigned long long)b.num_hash, (unsigned long long)b.k_size);
    printf("Number of accessions in index: %zu\n", b.colors.size());
    for (size_t c = 0; c < b.colors.size(); ++c)  // colour ids are already in sorted-name order
        printf("%s %llu %.3f\n", b.colors[c].c_str(), (unsigned long long)b.n_ref_kmers[c],
               false_prob((double)b.bloom_size, (double)b.num_hash, (double)b.n_ref_kmers[c]));
    return 0;
}

// the knobs read_id and batch_id share (main.rs:704-717 and :869-886 read the same flags with the same defaults)
struct ClassifyFlags {
    size_t down_sample, batch, bitvector_sample;
    double fp_correct;
    uint8_t quality;
};

ClassifyFlags classify_flags(const Args &a) {
    ClassifyFlags f;
    f.down_sample = num_or<size_t>(a, "down_sample", 1);
    f.fp_correct = std::pow(10.0, -num_or<double>(a, "fp_correct", 3.0));
    f.quality = num_or<uint8_t>(a, "quality", 15);
    f.batch = num_or<size_t>(a, "batch", 50000);
    f.bitvector_sample = num_or<size_t>(a, "bitvector_sample", 3);
    if (f.down_sample == 0 || f.batch == 0) die("attempt to calculate the remainder with a divisor of zero");
    return f;
}

bool one_gpu_run(const Args &a) { return !a.has("gpus") && !a.has("devices") && !a.has("placement") && !cli_env("COLORID_REDUCE"); }

// block-gzip input on one GPU goes up compressed and is inflated there (cid_fastq_*)
bool wants_device_front_end(const Args &a, const std::vector<std::string> &fq) {
    return ends_with(fq[0], ".gz") && one_gpu_run(a) && read_id_mt_pe::device_fastq_wanted(fq, fq.size() > 1 ? 2 : 1);
}

// --taxon TAXON [--exclude] [--gz-matches] (read_id, batch_id): the reference's read_filter fused into the classifying pass — the kept reads
// are cut and compressed on the device (cid_fastq_split with one bin; --gz-matches: with LZ77 matches, cid_fastq_filter_matches), so only
// block-gzip input on one GPU is served; everything else is refused here, before the GPU context is made.
// --split [--gz-matches]: every label's reads to a file of its own in the same pass (cid_fastq_split), the same route and the same refusals.
read_id_mt_pe::ReadOutput read_output(const Args &a) {
    read_id_mt_pe::ReadOutput f;
    const bool exclude = a.flags.count("exclude") != 0;
    const bool matches = a.flags.count("gz-matches") != 0;
    const bool split = a.flags.count("split") != 0;
    if (split && a.has("taxon")) die("error: --split writes every label's reads to a file of its own; --taxon TAXON writes one label's: give one of the two");
    if (split && exclude) die("error: --split writes every label's reads to a file of its own; --exclude belongs to --taxon TAXON: leave it out");
    if (exclude && !a.has("taxon")) die("error: --exclude needs --taxon TAXON (the classification to leave out)");
    if (matches && !a.has("taxon") && !split) die("error: --gz-matches needs --taxon TAXON or --split (it chooses how the reads written are compressed)");
    f.gz_matches = matches;
    if (split) { f.mode = f.kSplit; return f; }
    if (!a.has("taxon")) return f;
    f.mode = f.kTaxon; f.taxon = a.one("taxon"); f.exclude = exclude;
    return f;
}
void require_output_route(const Args &a, const std::vector<std::string> &fq, bool split) {
    if (wants_device_front_end(a, fq)) return;
    const char *why = !one_gpu_run(a) ? "it runs on one GPU only (no --gpus / --devices / --placement)"
                      : (cli_env("COLORID_DEVICE_FASTQ") && atoi(cli_env("COLORID_DEVICE_FASTQ")) == 0) ? "COLORID_DEVICE_FASTQ=0 turns the device front end off"
                      : !ends_with(fq[0], ".gz") ? "the input is not compressed"
                      : "the input is a single gzip stream, not block-gzip";
    die("error: %s in the classifying pass on the GPU, which takes block-gzip (BGZF) fastq input: %s; "
        "compress the reads with bgzip (%s)", split ? "--split writes every label's reads" : "--taxon writes the kept reads", why, fq[0].c_str());
}

// Start reading a sample's files before whoever classifies them asks: gzip decoding (or, for the device front end, reading the
// compressed members: a stretch or two, the reader's queue) then runs beside GPU start-up and the index load — measured against
// starting it after the context exists, the classification phase of 1 M reads ends 130 ms earlier — or, in batch_id, beside the
// tail of the sample before.
void read_ahead(const std::vector<std::string> &fq, bool device_front_end) {
    if (!ends_with(fq[0], ".gz")) return;
    for (size_t i = 0; i < fq.size() && i < 2; ++i) {
        if (device_front_end)
            BgzfMemberReader::prefetch(fq[i], read_id_mt_pe::device_fastq_stretch_bytes(0), read_id_mt_pe::device_fastq_host_share(),
                                       read_id_mt_pe::device_fastq_host_threads(fq.size() > 1 ? 2 : 1));
        else
            LineReader::prefetch(fq[i]);
    }
}

// one sample through the classifier: PREFIX_reads.txt, then PREFIX_counts.txt from it (main.rs:790-866, read_id_batch.rs:37-95)
void classify_sample(cid_ctx *ctx, Bigsi &b, const std::vector<std::string> &fq, const std::string &prefix, const ClassifyFlags &f) {
    if (ends_with(fq[0], ".gz")) {
        if (fq.size() > 1) read_id_mt_pe::per_read_stream_pe(ctx, fq, b, f.down_sample, f.fp_correct, f.batch, prefix, f.quality, f.bitvector_sample);
        else read_id_mt_pe::per_read_stream_se(ctx, fq, b, f.down_sample, f.fp_correct, f.batch, prefix, f.quality, f.bitvector_sample);
    } else {
        read_id_mt_pe::stream_fasta(ctx, fq, b, f.down_sample, f.fp_correct, f.batch, prefix, f.bitvector_sample);
    }
    phase_done("classification");
    read_counts_five_fields(prefix + "_reads.txt", prefix);
    phase_done("counts file");
}

int cmd_read_id(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'q', "query", true, true}, {'c', "batch", true, false},
                                                     {'t', "threads", true, false}, {'n', "prefix", true, false}, {'d', "down_sample", true, false},
                                                     {'H', "high_mem_load", false, false}, {'p', "fp_correct", true, false},
                                                     {'Q', "quality", true, false}, {'B', "bitvector_sample", true, false},
                                                     {0, "taxon", true, false}, {0, "exclude", false, false},
                                                     {0, "gz-matches", false, false}, {0, "split", false, false}}));
    for (const char *req : {"bigsi", "query", "prefix"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const std::vector<std::string> fq = a.values.at("query");
    const ClassifyFlags flags = classify_flags(a);
    const std::string prefix = a.one("prefix");
    const read_id_mt_pe::ReadOutput output = read_output(a);
    const bool split = output.mode == output.kSplit;
    if (output.mode != output.kNone) require_output_route(a, fq, split);
    read_id_mt_pe::set_read_output(output);
    if (cli_env("COLORID_GPU_INFLATE") && atoi(cli_env("COLORID_GPU_INFLATE")) > 0) LineReader::inflate_on_gpu(num_or<int>(a, "device", 0));
    const bool device_front_end = wants_device_front_end(a, fq);
    read_ahead(fq, device_front_end);
    Gpus gpus = make_gpus(a);
    phase_done("GPU context");
    std::thread warm = warm_async(gpus, CID_WARM_READID | (device_front_end ? CID_WARM_INFLATE | CID_WARM_FASTQ : 0u));
    cid_ctx *ctx = gpus.ctx;
    Bigsi b = load_index(ctx, a, false, &gpus);
    replicate(gpus, b);
    warm.join();
    phase_done("index load");
    if (split) read_id_mt_pe::split_prepare(b, fq.size() > 1 ? 2 : 1);
    classify_sample(ctx, b, fq, prefix, flags);
    LineReader::drop_prefetched();
    BgzfMemberReader::drop_prefetched();
    release(gpus, b);
    phase_done("release");
    return 0;
}

// batch_id (main.rs:869-888 -> read_id_batch.rs:7-181): a sample sheet `name \t reads1 [\t reads2]`; the index is loaded ONCE and
// every sample goes through read_id's streamers with the prefix NAME_TAG.  The reference walks its FnvHashMap of samples in
// hash order; here they go in name order — every sample writes its own two files, so the order shows only on stderr.
// On this machine the point of the subcommand is the fixed cost: one GPU context and one index upload for the whole sheet,
// and the next sample's files are read ahead while the current one is classified.
int cmd_batch_id(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'q', "query", true, false}, {'T', "tag", true, false},
                                                     {'c', "batch", true, false}, {'t', "threads", true, false}, {'d', "down_sample", true, false},
                                                     {'H', "high_mem_load", false, false}, {'p', "fp_correct", true, false},
                                                     {'Q', "quality", true, false}, {'B', "bitvector_sample", true, false},
                                                     {0, "taxon", true, false}, {0, "exclude", false, false},
                                                     {0, "gz-matches", false, false}, {0, "split", false, false}}));
    for (const char *req : {"bigsi", "query", "tag"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    const ClassifyFlags flags = classify_flags(a);
    const std::string tag = a.one("tag");
    const auto sheet = tab_to_map(a.one("query"));
    std::vector<std::pair<std::string, std::vector<std::string>>> samples(sheet.begin(), sheet.end());
    const read_id_mt_pe::ReadOutput output = read_output(a);
    const bool split = output.mode == output.kSplit;
    if (output.mode != output.kNone) for (const auto &sm : samples) require_output_route(a, sm.second, split);
    read_id_mt_pe::set_read_output(output);
    if (cli_env("COLORID_GPU_INFLATE") && atoi(cli_env("COLORID_GPU_INFLATE")) > 0) LineReader::inflate_on_gpu(num_or<int>(a, "device", 0));
    std::vector<char> on_device(samples.size(), 0);
    bool any_on_device = false;
    for (size_t i = 0; i < samples.size(); ++i) any_on_device |= (on_device[i] = wants_device_front_end(a, samples[i].second));
    if (!samples.empty()) read_ahead(samples[0].second, on_device[0]);
    Gpus gpus = make_gpus(a);
    phase_done("GPU context");
    std::thread warm = warm_async(gpus, CID_WARM_READID | (any_on_device ? CID_WARM_INFLATE | CID_WARM_FASTQ : 0u));
    cid_ctx *ctx = gpus.ctx;
    Bigsi b = load_index(ctx, a, false, &gpus);
    replicate(gpus, b);
    warm.join();
    phase_done("index load");
    if (split) {
        size_t most = 1;
        for (const auto &sm : samples) most = std::max<size_t>(most, sm.second.size() > 1 ? 2 : 1);
        read_id_mt_pe::split_prepare(b, most);
    }
    for (size_t i = 0; i < samples.size(); ++i) {
        fprintf(stderr, "Classifying %s\n", samples[i].first.c_str());
        if (i + 1 < samples.size()) read_ahead(samples[i + 1].second, on_device[i + 1]);
        classify_sample(ctx, b, samples[i].second, samples[i].first + "_" + tag, flags);
    }
    LineReader::drop_prefetched();
    BgzfMemberReader::drop_prefetched();
    release(gpus, b);
    phase_done("release");
    return 0;
}

// Which hash variant was this index built with?  The .bxi/.mxi format has no hash id and the reference hashes with a 2019 crate
// (xxh3 ^0.1.1, Cargo.toml:9; call sites src/simple_bloom.rs:19-38) that cannot run here.  A Bloom filter has no false negatives:
// under the RIGHT variant every k-mer of an accession's own sequence file has all its n rows set in the accession's colour
// (src/build.rs:54-99 inserted exactly those k-mers), under a wrong one only the fraction ~ (row density)^n does.  For every
// variant and every accession of the reference list (`-r`, the file `build` was given) this prints that fraction.
int cmd_hashcheck(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, with_common({{'b', "bigsi", true, false}, {'r', "refs", true, false}, {'Q', "quality", true, false}}));
    for (const char *req : {"bigsi", "refs"})
        if (!a.has(req)) die("error: The following required arguments were not provided: --%s", req);
    if (a.has("hash")) die("hashcheck tries every variant: --hash is not accepted");
    cid_ctx *ctx = make_ctx(a);
    fprintf(stderr, "Loading index\n");
    Bigsi b = read_bigsi(ctx, a.one("bigsi"), CID_HASH_XXH3_V08, false);
    std::vector<double> worst(CID_HASH_VARIANTS, 2.0);
    const size_t n_checked = hashcheck(ctx, b, a.one("refs"), num_or<uint8_t>(a, "quality", 15), kHashNames, worst);
    if (n_checked == 0) die("no accession of %s is a colour of %s", a.one("refs").c_str(), a.one("bigsi").c_str());
    int match = -1, n_match = 0;
    for (int v = 0; v < CID_HASH_VARIANTS; ++v)
        if (worst[v] >= 0.999) { match = v; ++n_match; }
    if (n_match == 1) printf("verdict\t%s\tevery accession's own k-mers are present: use --hash %s\n", kHashNames[match], kHashNames[match]);
    else if (n_match == 0) printf("verdict\tnone\tno available hash variant reproduces this index (lowest fractions:");
    else printf("verdict\tambiguous\tmore than one variant fits (index too dense to tell)\n");
    if (n_match == 0) {
        for (int v = 0; v < CID_HASH_VARIANTS; ++v) printf(" %s %.4f", kHashNames[v], worst[v]);
        printf(")\n");
    }
    cid_index_destroy(b.index);
    cid_ctx_destroy(ctx);
    return n_match == 1 ? 0 : 3;
}

// host-only helper used by the CPU tests: distinct canonical k-mers of a file as "kmer\tcount" lines (insertion order)
int cmd_debug_kmers(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'q', "query", true, true}, {'k', "kmer", true, false}, {0, "mode", true, false},
                                         {'Q', "quality", true, false}, {'f', "filter", true, false}});
    KmerMap km(num_or<uint32_t>(a, "kmer", 31));
    const std::string mode = a.has("mode") ? a.one("mode") : "vector";
    const std::vector<std::string> q = a.values.at("query");
    if (mode == "vector") kmerize_vector(read_fasta(q[0]), 1, km);
    else if (mode == "fq") kmers_from_fq_qual(q[0], num_or<uint8_t>(a, "quality", 15), km);
    else if (mode == "fqpe") kmers_fq_pe_qual(q[0], q[1], num_or<uint8_t>(a, "quality", 15), km);
    else if (mode == "mf") {
        std::vector<std::string> labels, seqs;
        read_fasta_mf(q[0], labels, seqs);
        for (size_t i = 0; i < labels.size() && i < seqs.size(); ++i) {
            KmerMap one(km.k());
            printf(">%s\t%d\n", labels[i].c_str(), kmerize_string(seqs[i], one) ? (int)one.size() : -1);
        }
        return 0;
    } else die("unknown mode");
    if (a.has("filter")) {
        const int64_t f = num_or<int64_t>(a, "filter", 0);
        if (f < 0) { const int64_t t = km.auto_cutoff(); printf("#auto_cutoff\t%lld\n", (long long)t); if (t >= 0) km.clean((uint64_t)t); }
        else km.clean((uint64_t)f);
    }
    for (size_t e = 0; e < km.size(); ++e) {
        fwrite(km.keys() + e * km.k(), 1, km.k(), stdout);
        printf("\t%u\n", km.counts()[e]);
    }
    return 0;
}

// host-only helper used by the CPU tests: the reads of a FASTQ file (pair) as the record pipeline packs them for read_id / search
int cmd_debug_records(int argc, char **argv) {
    const Args a = parse(argc, argv, 2, {{'q', "query", true, true}, {'Q', "quality", true, false}});
    const std::vector<std::string> q = a.values.at("query");
    debug_records(q[0], q.size() > 1 ? &q[1] : nullptr, num_or<uint8_t>(a, "quality", 15));
    return 0;
}

// the end of a subcommand: everything it printed leaves the stdio buffers, then the process ends without the teardown (see release())
int leave(int rc) {
    phase_done("subcommand returned");
    // a result that did not reach its pipe or disk is a failed run, whichever way the process leaves (EX_IOERR)
    const bool lost = fflush(nullptr) != 0 || ferror(stdout);
    if (lost) {
        fprintf(stderr, "colorid: writing the output failed: %s\n", strerror(errno));
        if (rc == 0) rc = 74;
    }
    if (!g_orderly_exit) _exit(rc);
    return rc;
}

}  // namespace

int main(int argc, char **argv) {
    // src/main.rs:16-20: init_log() prints this banner on stdout before anything else
    printf("\n ************** initializing logger *****************\n\n");
    if (argc < 2) {
        fprintf(stderr, "colorid 0.1.4.3 (MI355X)\nUSAGE:\n    colorid <build|search|info|read_id|batch_id|hashcheck|merge|subset|fold|compare|collapse|dists|alleles> [FLAGS]\n");
        return 1;
    }
    const std::string cmd = argv[1];
    if (cmd == "--help" || cmd == "-h" || cmd == "help") {
        printf("colorid 0.1.4.3 (MI355X)\nUSAGE:\n    colorid <build|search|info|read_id|batch_id|hashcheck|merge|subset|fold|compare|collapse|dists|alleles> [FLAGS]      (flags: colorid <subcommand> --help)\n\n"
               "SEARCH:\n"
               "    search -b idx.bxi -q R1.fq.gz [-r R2.fq.gz] [-f N] --gather PREFIX [--gather-min 1000] [--gather-max R]   the usual rows, and\n"
               "                             PREFIX.gather.tsv: the accessions that explain the sample, greedily — the one with most of the\n"
               "                             sample's k-mers, then the one with most of what is left, ... until an accession adds fewer than\n"
               "                             --gather-min k-mers or --gather-max rows are out; shared k-mers count once; one GPU, at most\n"
               "                             8192 accessions\n"
               "    search -b idx.bxi -q panel.fasta -g -m [-p 0.35]               every FASTA record its own gene query\n"
               "    search -b idx.bxi -q panel.fasta -g -m --coverage [-p 0.35]    the same rows, and where on the record the accession hits:\n"
               "                             bases covered / record length, longest covered stretch (bases), stretches, first and last\n"
               "                             covered base (1-based); one GPU, FASTA queries, at most 8192 accessions\n"
               "    search -b idx.bxi -q scheme.fasta -s -m --alleles PREFIX [--max-missing N]   the rows of -s -m (every record an allele\n"
               "                             named LOCUS_ALLELE), and from them the accessions x loci table: PREFIX.raw.tsv (allele, or NA for\n"
               "                             several or none), PREFIX.detailed.tsv (MULTI / NOT_CALLED), PREFIX.report.out; --max-missing N:\n"
               "                             PREFIX.clean.tsv without, PREFIX.dropped.txt with the accessions of more than N NA cells\n"
               "    search -b idx.bxi -q scheme.fasta -s -m --alleles PREFIX --nearest [-p 0.35]   also PREFIX.nearest.tsv: for every accession\n"
               "                             and locus without a perfect allele, the known allele that shares most of its k-mers with the\n"
               "                             accession (share >= -p): a novel allele shares > 0.9, an absent locus nothing; one GPU, at most\n"
               "                             8192 accessions\n"
               "    search -b idx.bxi -q scheme.fasta -s -m --alleles PREFIX --dists [--cluster T [--min-compared M]]   also PREFIX.dists.tsv and\n"
               "                             PREFIX.compared.tsv: for every two accessions of the raw table (of the clean one with --max-missing)\n"
               "                             the loci where both have an allele and the alleles differ / where both have one; --cluster T:\n"
               "                             PREFIX.clusters.tsv, single linkage of the pairs at most T loci apart that share at least M (1)\n"
               "                             --dists --mst [--min-compared M]: PREFIX.mst.tsv and PREFIX.mst.nwk, the minimum spanning forest over\n"
               "                             the pairs that share at least M (1) loci: fewest differing loci first, then most shared loci, then\n"
               "                             the earlier accessions; edges a, b, differ, compared and one Newick line per tree (branch length =\n"
               "                             differing loci); its edges of at most T are the clusters of --cluster T.  --no-matrices (with --mst\n"
               "                             or --cluster): PREFIX.dists.tsv and PREFIX.compared.tsv are not written\n"
               "                             --dists --within T [--min-compared M]: PREFIX.within.tsv, a, b, differ, compared for every two\n"
               "                             accessions that share at least M (1) loci and differ at no more than T of them, a before b in the\n"
               "                             table: the pairs are found on the GPU and only they come back (goes with --no-matrices); their\n"
               "                             connected components are the clusters of --cluster T\n"
               "                             --dists --closest K [--within T] [--min-compared M]: PREFIX.closest.tsv, accession, neighbour, differ,\n"
               "                             compared: under every accession its K (1 .. 64) nearest among those that share at least M (1) loci\n"
               "                             with it (and differ at no more than T), fewest differing loci first, then most shared loci, then\n"
               "                             table order; a line of - for none; found on the GPU, no matrix is made (goes with --no-matrices)\n"
               "                             --dists --hist [--min-compared M]: PREFIX.hist.tsv, loci, differ_pairs, differ_cumulative,\n"
               "                             compared_pairs: for n = 0 .. the number of loci, the unordered pairs that share at least M (1) loci\n"
               "                             and differ at exactly n, their running sum (the lines --within n would write), and the pairs that\n"
               "                             share exactly n loci: where to put T and M; counted on the GPU (goes with --no-matrices)\n"
               "                             --dists --levels T1,T2,.. [--min-compared M]: PREFIX.levels.tsv, accession, one column T<t> per\n"
               "                             threshold (1 .. 32 of them, coarse to fine) = the cluster column of --cluster t, and address, the\n"
               "                             numbers joined by '.': all from the one minimum spanning forest (goes with --no-matrices)\n"
               "    dists -t TABLE -o PREFIX [--cluster T] [--mst] [--min-compared M] [--no-matrices]   the same files from a table in the form\n"
               "                             of PREFIX.raw.tsv; [--within T] [--closest K] [--hist] [--levels T1,T2,..] as above\n"
               "    dists -t TABLE --query TABLE2 -o PREFIX --within T [--min-compared M]   PREFIX.query.tsv alone: for every accession of TABLE2\n"
               "                             the accessions of TABLE and of TABLE2 within T, nearest first (query, neighbour, in = table or\n"
               "                             query, differ, compared; a line of - for none); loci are matched by name: TABLE's are used, one that\n"
               "                             TABLE2 lacks is no call there, one only TABLE2 has is ignored\n"
               "    dists -t TABLE --query TABLE2 -o PREFIX --closest K [--within T] [--min-compared M]   the same file, every list cut to its K\n"
               "                             nearest; without --within however far they are\n"
               "    alleles -r ROWS -o PREFIX [--max-missing N]   the same tables from the saved stdout of a `search -s -m` run; no GPU\n\n"
               "INDEX MAINTENANCE:\n"
               "    collapse -b OUT -i idx.bxi -g groups.tsv      several accessions as one colour (groups.tsv: accession TAB group per line;\n"
               "                             unlisted accessions stay as they are, a group of one is a rename): rows are the OR of the\n"
               "                             members' rows, n_ref_kmers is estimated from fill; OUT_groups.tsv reports fill and\n"
               "                             false-positive rates per group (see fold -p); one GPU\n\n"
               "ENVIRONMENT:\n"
               "    COLORID_FAST_EXIT=1      leave without the GPU runtime's teardown once the results are written, closed and flushed\n"
               "                             (-0.05 to -0.15 s per run); =0, or COLORID_FULL_TEARDOWN=1: always the orderly exit\n"
               "                             unset: the short way, unless a preloaded library, a profiler's tool library or coverage\n"
               "                             counters are present (they write at exit) or several GPUs are in use (RCCL is shut down)\n"
               "                             this run would leave: %s (%s)\n"
               "    COLORID_INDEX_MMAP=0     read the index through a buffered reader instead of a mapping\n"
               "    COLORID_DEVICE_FASTQ=0   FASTQ text on the host front end only\n",
               g_orderly_exit ? "the orderly way" : "the short way", g_exit_reason);
        return 0;
    }
    if (cmd == "build") return leave(cmd_build(argc, argv));
    if (cmd == "search") return leave(cmd_search(argc, argv));
    if (cmd == "info") return leave(cmd_info(argc, argv));
    if (cmd == "read_id") return leave(cmd_read_id(argc, argv));
    if (cmd == "hashcheck") return leave(cmd_hashcheck(argc, argv));
    if (cmd == "merge") return leave(cmd_merge(argc, argv));
    if (cmd == "subset") return leave(cmd_subset(argc, argv));
    if (cmd == "fold") return leave(cmd_fold(argc, argv));
    if (cmd == "compare") return leave(cmd_compare(argc, argv));
    if (cmd == "collapse") return leave(cmd_collapse(argc, argv));
    if (cmd == "dists") return leave(cmd_dists(argc, argv));
    if (cmd == "alleles") return leave(cmd_alleles(argc, argv));
    if (cmd == "debug-kmers") return cmd_debug_kmers(argc, argv);
    if (cmd == "debug-records") return cmd_debug_records(argc, argv);
    if (cmd == "batch_id") return leave(cmd_batch_id(argc, argv));
    if (cmd == "read_filter") die("'%s' is outside the accelerated query path; use the reference binary", cmd.c_str());
    die("error: Found argument '%s' which wasn't expected", cmd.c_str());
}
