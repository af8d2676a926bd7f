// Host side of colorid's query path, C++17, above the C ABI (include/colorid_hip.h).
// The reference host is Rust (no toolchain in this image); names and argument meaning follow the reference
// functions cited at each declaration so the call sites read like src/main.rs.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <thread>
#include <unordered_map>
#include <mutex>
#include <functional>
#include <deque>
#include <condition_variable>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../../../include/colorid_hip.h"

namespace colorid {

[[noreturn]] void die(const char *fmt, ...);  // the reference panics (expect/unwrap): message + exit code 101
// An output that is only valid once finished (--taxon's .fq.gz: whole members without the end-of-file block pass gzip -t): from
// remove_on_die until keep_on_die, die() on any thread unlinks it before the process leaves.
void remove_on_die(const std::string &path);
void keep_on_die(const std::string &path);

// ---------------------------------------------------------------- seq.rs / kmer.rs (query side)
std::vector<std::string> read_fasta(const std::string &path);                                          // kmer.rs:10-45
void read_fasta_mf(const std::string &path, std::vector<std::string> &labels, std::vector<std::string> &seqs);  // kmer.rs:47-84
void qual_mask(std::string &seq, const std::string &qual, uint8_t q);                                  // seq.rs:36-56 (in place)

// FnvHashMap<String, usize> of canonical k-mers: packed keys (n * k bytes) + counts.  Iteration order is
// insertion order (the reference's is arbitrary).
class KmerMap {
  public:
    explicit KmerMap(uint32_t k);
    uint32_t k() const { return k_; }
    size_t size() const { return counts_.size(); }
    const uint8_t *keys() const { return keys_.data(); }
    const std::vector<uint32_t> &counts() const { return counts_; }
    void add(const uint8_t *key, uint32_t n = 1);
    void clean(uint64_t t);          // kmer.rs:826-837: keep count > t
    int64_t auto_cutoff() const;     // kmer.rs:866-942; -1 where the reference would panic
  private:
    void rehash();
    uint32_t k_;
    std::vector<uint8_t> keys_;
    std::vector<uint32_t> counts_;
    std::vector<uint32_t> table_;  // entry + 1
};
// kmer.rs:866-942 on the histogram {multiplicity -> number of distinct k-mers}; -1 where the reference would panic
int64_t auto_cutoff_from_histogram(const std::map<uint64_t, uint64_t> &histo, uint64_t n_distinct);
void kmerize_vector(const std::vector<std::string> &v, size_t d, KmerMap &out);   // kmer.rs:87-125
bool kmerize_string(const std::string &l, KmerMap &out);                          // kmer.rs:271-299 (false = None)
// kmerize_vector({seq}, 1, out) with every window kept in place: k bytes (the k-mer, or filler for a window with a non-ACGT base) and one
// flag byte (CID_WIN_VALID, CID_WIN_FIRST) per window, appended to keys / flags (`search -g -m --coverage`)
void kmerize_windows(const std::string &seq, KmerMap &out, std::vector<uint8_t> &keys, std::vector<uint8_t> &flags);
void kmers_from_fq_qual(const std::string &path, uint8_t q, KmerMap &out);        // kmer.rs:461-510
void kmers_fq_pe_qual(const std::string &p1, const std::string &p2, uint8_t q, KmerMap &out);  // kmer.rs:581-655

// CPUs this process may keep busy: the cgroup's CPU quota (cpu.max) when there is one, else the hardware's thread count.  The
// host pipeline sizes its pools from it (a third for inflating block-gzip members, a fifth for packing records): more runnable threads than the quota get the whole process throttled for the rest of the scheduling period, which on a
// 16-CPU share of a GPU box cost more than the extra threads brought (tools/exp_readid_stages.sh).
int cpu_budget();

// A few persistent worker threads.  The pipeline used to start threads per batch (inflating a batch's members, packing a chunk's
// records, polling a batch's slices): a thread's start and end map and unmap its stack, and in a process whose other threads fault
// pages all the time those calls queue on the address-space lock — two poll threads per batch were twice as SLOW as one.
// The command line's environment switches (cli_switches.def lists them; README.md's table is generated from it): cli_env("NAME") returns
// the variable's value as it was when the first switch was asked for — one snapshot of the listed names, whoever asks — or nullptr.
inline const char *cli_env(const char *name) {
    struct Snapshot {
        std::vector<std::pair<std::string, std::string>> set;   // the listed variables that are set
        std::vector<std::string> known;
        Snapshot() {
#define CLI_SWITCH(id, env, kind, dflt, doc) known.push_back(env); if (const char *e = getenv(env)) set.emplace_back(env, e);
#include "cli_switches.def"
#undef CLI_SWITCH
        }
    };
    static const Snapshot snap;
    for (const auto &kv : snap.set) if (kv.first == name) return kv.second.c_str();
    for (const auto &k : snap.known) if (k == name) return nullptr;
    fprintf(stderr, "cli_env: '%s' is not in cli_switches.def\n", name);
    abort();
}

class TaskPool {
  public:
    explicit TaskPool(int n_threads) {
        for (int i = 0; i < n_threads; ++i) threads_.emplace_back([this] { run(); });
    }
    ~TaskPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    TaskPool(const TaskPool &) = delete;
    TaskPool &operator=(const TaskPool &) = delete;
    void submit(std::function<void()> fn) {
        { std::lock_guard<std::mutex> lk(mu_); q_.push_back(std::move(fn)); }
        cv_.notify_one();
    }
    // fn(0) .. fn(n-1), the caller taking part; returns when all are done
    void parallel_for(size_t n, const std::function<void(size_t)> &fn) {
        if (n == 0) return;
        struct Latch { std::mutex m; std::condition_variable c; size_t left; } latch;
        latch.left = n - 1;
        for (size_t i = 1; i < n; ++i)
            submit([&fn, &latch, i] {
                fn(i);
                std::lock_guard<std::mutex> lk(latch.m);
                if (--latch.left == 0) latch.c.notify_one();
            });
        fn(0);
        std::unique_lock<std::mutex> lk(latch.m);
        latch.c.wait(lk, [&] { return latch.left == 0; });
    }
  private:
    void run() {
        for (;;) {
            std::function<void()> fn;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                fn = std::move(q_.front());
                q_.pop_front();
            }
            fn();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    std::vector<std::thread> threads_;
    bool stop_ = false;
};

// gz/plain line reader with BufRead::lines() semantics (strips \n and \r\n)
class LineReader {   // inflates on its own thread, a few MiB ahead of the caller (two mates of a pair decode in parallel)
  public:
    explicit LineReader(const std::string &path);
    ~LineReader();
    // Start inflating `path` now, up to ~256 MiB of text ahead: the next LineReader opened on the same path takes the stream
    // over.  The CLI calls this before it loads the index, so that gzip decoding runs beside the index load instead of after it.
    static void prefetch(const std::string &path);
    static void drop_prefetched();   // end of a command: stop the streams nobody took
    static double blocked_ms();      // COLORID_TIMING: time the decoding threads waited for their consumer (all readers so far)
    // Block-gzip (BGZF) input is inflated on GPU `device` (cid_bgzf_inflate: one wave per member) instead of on COLORID_GZ_THREADS
    // host threads; < 0 = on the host.  Applies to readers opened afterwards; each reader thread uses a context of its own.
    static void inflate_on_gpu(int device);
    LineReader(const LineReader &) = delete;
    LineReader &operator=(const LineReader &) = delete;
    bool next(std::string &line);
    // the same line as a view: valid until the next call on this reader (it points into the decoded block, or into the reader's
    // own buffer for a line that straddles two blocks) — no per-line copy
    bool next(const char *&ptr, size_t &len);
    // Block interface, for a caller that splits the text itself (RecordChunker; not to be mixed with next() on one reader): the
    // next decoded block, its text at [kHeadroom, blk.size()) — the bytes in front are the caller's to fill (the tail of the
    // previous block).  Blocks go back with recycle().
    static constexpr size_t kHeadroom = 1u << 16;
    bool next_block(std::vector<char> &blk);
    void recycle(std::vector<char> &&blk);
    struct Impl;   // (defined in fastx_kmers.cpp)
  private:
    Impl *p_;
};

// Whole FASTQ records (groups of four lines, counted from the start of the file as the reference's `line_count % 4` does) of one
// Block-gzip (BGZF) input for the device front end (cid_fastq_*): the file's members still COMPRESSED, in stretches worth about
// `text_target` bytes of text — the reading thread only walks the members' headers (their sizes are in the "BC" extra field, the
// text sizes in the trailers) a stretch or two ahead of the caller; inflate, line split, record split and masking happen on the GPU.
struct ByteBuf {   // a growable byte buffer that never zero-fills what it is about to overwrite (fread targets of tens of MB)
    unsigned char *p = nullptr;
    size_t n = 0, cap = 0;
    ByteBuf() = default;
    ByteBuf(const ByteBuf &) = delete;
    ByteBuf &operator=(const ByteBuf &) = delete;
    ByteBuf(ByteBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    ByteBuf &operator=(ByteBuf &&o) noexcept { if (this != &o) { free(p); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = o.cap = 0; } return *this; }
    ~ByteBuf() { free(p); }
    void reserve(size_t want) {
        if (want <= cap) return;
        size_t c = cap ? cap : (size_t)1 << 20;
        while (c < want) c += c / 2;
        unsigned char *q = static_cast<unsigned char *>(realloc(p, c));
        if (!q) die("out of memory (%zu bytes)", c);
        p = q; cap = c;
    }
    unsigned char *data() { return p; }
    const unsigned char *data() const { return p; }
    size_t size() const { return n; }
};
struct PinnedBuf {   // page-locked bytes from the library (cid_pinned_alloc; plain malloc when that fails), grown, never shrunk
    unsigned char *p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.cap = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; pinned = o.pinned; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinnedBuf() { release(); }
    void release();
    void reserve(size_t want);   // (contents are not kept)
};
struct StretchBuf {   // a stretch's compressed bytes: page-locked when the library hands such memory out, grown with its contents kept
    unsigned char *p = nullptr;
    size_t n = 0, cap = 0;
    bool pinned = false;
    StretchBuf() = default;
    StretchBuf(const StretchBuf &) = delete;
    StretchBuf &operator=(const StretchBuf &) = delete;
    StretchBuf(StretchBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.n = o.cap = 0; }
    StretchBuf &operator=(StretchBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; cap = o.cap; pinned = o.pinned; o.p = nullptr; o.n = o.cap = 0; }
        return *this;
    }
    ~StretchBuf() { release(); }
    void release();
    void reserve(size_t want);   // (the first n bytes are kept)
    unsigned char *data() { return p; }
    const unsigned char *data() const { return p; }
    size_t size() const { return n; }
};
struct BgzfStretch {
    // Whole members, back to back.  COLORID_DEVICE_FASTQ_PINNED=1 puts them in page-locked memory, sized once per stretch (from the file's
    // size, then from the stretch before), and their copy to the device then runs beside the loop (CID_FASTQ_KEEP): the push of 16 M
    // reads falls from 150-190 ms to 14-36 — and the loop stays where it was, 296-310 ms against 307-315, because the GPU is what it
    // waits for by then (k_bgzf_inflate_wave 10 ms and k_readid 9.6 ms per 256 MiB stretch, side by side 13.3: rocprofv3 of the command
    // line, profiles/r06_frontend_gpu_bound.txt), while two files of pairs start 25-35 ms later behind their larger first buffers
    // (4 M pairs 139-142 ms against 97-104).  Off by default.
    StretchBuf bytes;
    std::vector<uint32_t> off, len, text_len;      // member i = bytes[off[i], +len[i]), its text has text_len[i] bytes
    uint64_t text_bytes = 0;
    bool last = false;                             // the file ends with this stretch
    // the members [device_members, off.size()) are inflated already, by the reader's host threads: their text, back to back
    size_t device_members = 0;
    PinnedBuf host_text;
    size_t host_text_bytes = 0;
};
class BgzfMemberReader {
  public:
    // host_share: the fraction of every stretch's text that `host_threads` threads of the reader inflate themselves (0: none)
    BgzfMemberReader(const std::string &path, size_t text_target, double host_share = 0.0, int host_threads = 0);
    ~BgzfMemberReader();
    BgzfMemberReader(const BgzfMemberReader &) = delete;
    BgzfMemberReader &operator=(const BgzfMemberReader &) = delete;
    bool next(BgzfStretch &s);                     // false after the stretch that had last == true; `s`'s buffers are recycled
    static bool is_bgzf(const std::string &path);
    // Start reading `path` now (the CLI calls this before the GPU context and the index exist); open() hands the running reader over
    // — or starts one — to whoever classifies the file.  drop_prefetched(): readers nobody took.
    static void prefetch(const std::string &path, size_t text_target, double host_share, int host_threads);
    static std::unique_ptr<BgzfMemberReader> open(const std::string &path, size_t text_target, double host_share, int host_threads);
    static void drop_prefetched();
    size_t text_target() const;
    struct Impl;
  private:
    Impl *p_;
};

// input, a decoded block at a time: the text [begin, rec_end.back()) of buf, record r ending just past its fourth newline at
// rec_end[r].  Lines that do not complete a record at the end of the input are dropped, as the line loops never push them
// (read_id_mt_pe.rs:862-895).  Finding the boundaries is one memchr per line; the records of a chunk are then parsed in parallel.
struct RecChunk {
    std::vector<char> buf;
    size_t begin = 0;
    std::vector<uint32_t> rec_end;
    size_t records() const { return rec_end.size(); }
    size_t rec_begin(size_t r) const { return r ? rec_end[r - 1] : begin; }
};
class RecordChunker {
  public:
    explicit RecordChunker(LineReader &r) : r_(r) {}
    bool next(RecChunk &c);              // false at the end of the input
    void recycle(RecChunk &c) { if (!c.buf.empty()) r_.recycle(std::move(c.buf)); c.buf = std::vector<char>(); c.rec_end.clear(); }
  private:
    LineReader &r_;
    std::string carry_;                  // the lines after the last whole record of the previous block
    uint64_t carry_lines_ = 0;           // newlines inside carry_
    bool done_ = false;
};

void debug_records(const std::string &f1, const std::string *f2, uint8_t q);   // CPU tests: the reads as the record pipeline packs them

// GPU k-mer maps (cid_kmerset, k <= 32; COLORID_HOST_KMERS=1 forces the host map).  count_fastq_gpu returns nullptr when
// the file holds lower-case bases (their case is kept, so they cannot be packed): the caller counts on the host.
bool gpu_counting_enabled(uint64_t k);
// `target`: the index the set is going to be searched in (cid_kmerset_set_target_index: ordered for it at no extra pass); null = code order
cid_kmerset *count_fasta_gpu(cid_ctx *ctx, uint64_t k, const std::vector<std::string> &seqs, const cid_index *target = nullptr);
cid_kmerset *count_fastq_gpu(cid_ctx *ctx, uint64_t k, const std::string &f1, const std::string *f2, uint8_t q, const cid_index *target = nullptr);
int64_t auto_cutoff_gpu(cid_kmerset *ks);   // kmer.rs:866-942 from the device histogram

// ---------------------------------------------------------------- bigsi.rs
struct Bigsi {  // BigsyMapNew minus the map, which lives on the device
    uint64_t bloom_size = 0, num_hash = 0, k_size = 0;
    uint64_t m_size = 0;                    // > 0: BigsyMapMiniNew (.mxi), Bloom keys are minimizers of this length
    std::vector<std::string> colors;        // colour id -> accession
    std::vector<uint64_t> n_ref_kmers;      // by colour id
    cid_index *index = nullptr;
};
// stripes != nullptr: the index goes to the ranks of `group` as colour stripes (cid_group_stripes_*) instead of to one GPU; b.index stays null
Bigsi read_bigsi(cid_ctx *ctx, const std::string &path, int hash_variant, bool meta_only = false, cid_group *group = nullptr,
                 std::vector<cid_index *> *stripes = nullptr);  // bigsi.rs:59-69
// map the index file and start touching its pages — call it before the GPU context is made; read_bigsi then uploads from the mapping
void bigsi_read_ahead(const std::string &path);
void save_bigsi(const std::string &path, const Bigsi &b);                                           // bigsi.rs:51-57
// The input index of a command that streams row records (`merge`, `subset`, `compare`, `fold`, `collapse`), as the command's _check read it
struct IndexInput {
    std::string path;
    Bigsi meta;          // header, colours and n_ref_kmers; no device index
    uint64_t n_rows = 0;
};
// `merge` (no reference counterpart): indices of one shape and disjoint accessions as one index over the union of their accessions,
// colours in name order as `build` numbers them.  merge_check reads every input's header and n_ref_kmers (not its rows) and refuses,
// naming field or accession and files, what cannot be merged — before any GPU work; it returns the merged metadata (no index yet) and
// each input's colour map.  merge_records makes the index on ctx and ORs every input's row records into it (not finalized).
struct MergeInput : IndexInput {
    std::vector<uint32_t> colour_map;  // input colour -> merged colour (increasing)
};
Bigsi merge_check(const std::vector<std::string> &paths, const std::string &out_path, std::vector<MergeInput> &inputs);
void merge_records(cid_ctx *ctx, Bigsi &merged, const std::vector<MergeInput> &inputs);
// `subset` (no reference counterpart): the accessions of one index that a list names (exclude: all the others) as an index of their
// own — the file `build` writes over the kept lines of the reference list.  subset_check reads the header, the n_ref_kmers and the list
// (text, one accession per line up to the first TAB) and refuses before any GPU work, naming file and accession; it returns the output's
// metadata (no index yet) and the keep bitmap.  subset_records makes the index on ctx and streams the input's records through
// cid_index_put_records_subset (not finalized): the device holds the OUTPUT index and one upload chunk, never the input's matrix.
struct SubsetInput : IndexInput {
    std::vector<uint32_t> keep_words;  // bitmap over the input's colours, in the rows' bit order
};
Bigsi subset_check(const std::string &in_path, const std::string &out_path, const std::string &list_path, bool exclude, SubsetInput &in);
void subset_records(cid_ctx *ctx, Bigsi &out, const SubsetInput &in);
// `collapse` (no reference counterpart): several accessions of one index as one colour — the file `build` writes over a reference list
// with one line per group whose FASTA is the members' FASTA files joined (the Bloom filter of a union is the OR of the filters).  The
// groups file is text, `accession TAB group` per line; an accession it does not list stays a group of its own under its own name, so a
// listed accession alone in a group is a rename.  collapse_check reads the header, the n_ref_kmers tail and the groups file and refuses
// before any GPU work, naming file and accession or group; it returns the output's metadata — colours in byte order of the group names,
// n_ref_kmers still zero — and the map.  collapse_records makes the index on ctx, streams the input's records through
// cid_index_put_records_grouped (not finalized) and fills in the columns' bit counts and the output's n_ref_kmers (collapse_n_ref): the
// device holds the OUTPUT index and one upload chunk, never the input's matrix.
struct CollapseInput : IndexInput {
    std::vector<uint32_t> group_of;               // input colour -> output colour
    std::vector<std::vector<uint32_t>> members;   // output colour -> its input colours, ascending
    std::vector<uint64_t> bits_file, bits_index;  // set bits per input / output column (collapse_records)
};
Bigsi collapse_check(const std::string &in_path, const std::string &out_path, const std::string &groups_path, CollapseInput &in);
void collapse_records(cid_ctx *ctx, Bigsi &out, CollapseInput &in);
// The n_ref_kmers of a group: the union's size is not in the index, so it is estimated from fill.  est(X) = -(m/n) ln(1 - X/m) is the
// number of keys that set X of a filter's m bits with n hashes.  One member: its own count.  A member without a count (0: `build -m`
// from reads): 0.  A full column (X == m) among the members or the group: the sum of the members' counts.  Else
// round(sum n_i * est(X_group) / sum est(X_i)) — the ratio, since the keys of an .mxi are minimizers while n_ref_kmers counts k-mers —
// clamped to [max n_i, sum n_i].
uint64_t collapse_n_ref(uint64_t bloom_size, uint64_t num_hash, const std::vector<uint64_t> &n_i, const std::vector<uint64_t> &bits_i,
                        uint64_t bits_group);
// `compare` (no reference counterpart): which accessions of an index are (nearly) the same Bloom filter.  compare_check reads the header
// and the n_ref_kmers tail and refuses before any GPU work (file missing, truncated, an accession twice).  compare_records makes the pair
// counters on ctx, streams the input's records through cid_pairs_add_records and returns the symmetric n x n matrix shared[i][j] =
// popcount(column i & column j): the device holds the counters and one upload chunk, never the input's matrix.
using CompareInput = IndexInput;
void compare_check(const std::string &in_path, CompareInput &in);
std::vector<uint64_t> compare_records(cid_ctx *ctx, const CompareInput &in);
// `fold` (no reference counterpart): one index at a smaller Bloom size that divides its own — the file `build -s NEW` writes over the same
// reference list, made from the index alone (every row is hash % bloom_size, so row r of the input is OR-ed into row r % NEW).  The new
// size is given (by = 's'), or as the factor to divide by ('f'), or as the largest false-positive rate any accession may have ('p': the
// smallest divisor of the input's size at which false_prob, as `info` prints it, stays at or under the bound for every accession).
// fold_check reads the header and the n_ref_kmers tail and refuses before any GPU work, naming file and numbers; it returns the output's
// metadata (no index yet).  fold_records makes the index on ctx and streams the input's records through cid_index_put_records_folded
// (not finalized): the device holds the OUTPUT index and one upload chunk, never the input's matrix.
struct FoldInput : IndexInput {
    uint64_t factor = 0;      // input's bloom_size / the output's
    size_t worst = 0;         // the accession with the highest predicted false-positive rate at the output's size, and that rate
    double worst_fp = 0.0;
};
Bigsi fold_check(const std::string &in_path, const std::string &out_path, char by, const std::string &value, FoldInput &in);
void fold_records(cid_ctx *ctx, Bigsi &out, const FoldInput &in);
Bigsi build_single(cid_ctx *ctx, const std::string &ref_tsv, uint64_t bloom, uint64_t hashes, uint64_t k, uint8_t quality,
                   int64_t cutoff, int hash_variant, uint64_t m_size = 0);   // build.rs:15-130; m_size > 0: build_single_mini :396-492

// For every hash variant v and every accession of ref_tsv that is a colour of b: the fraction of the accession's k-mers (counted
// as build does, build.rs:54-99) whose n rows are all set in its colour.  Prints one line per (variant, accession); worst[v] = the
// smallest fraction under variant v.  Returns the number of accessions checked.
// build.rs:15-31: `name \t file [\t file2]` per line, a later line of the same name replaces the earlier one (the sample sheet of
// `build -r`, `hashcheck -r` and `batch_id -q`); iterated in name order
std::map<std::string, std::vector<std::string>> tab_to_map(const std::string &tsv);
size_t hashcheck(cid_ctx *ctx, Bigsi &b, const std::string &ref_tsv, uint8_t quality, const char *const *variant_names, std::vector<double> &worst);

// ---------------------------------------------------------------- reports.rs / read_id tail
double false_prob(double m, double k, double n);                                                     // read_id_mt_pe.rs:695-698
struct Classification { std::string label; uint64_t count; uint64_t kmer_length; const char *verdict; uint64_t n_top; };
// read_id_mt_pe.rs:187-251 on the report's non-zero entries (ascending colour id; colour C = no_hits_num)
Classification kmer_poll_plus(const uint32_t *colours, const uint32_t *counts, size_t n_entries, uint64_t kmer_length, const Bigsi &b,
                              const std::vector<double> &fp, double fp_correct);
void read_counts_five_fields(const std::string &reads_file, const std::string &prefix);            // reports.rs:98-120

// ---------------------------------------------------------------- allele table (alleles.cpp)
// `search -s -m` rows -> the accessions x loci table of a cgMLST scheme (PREFIX.raw.tsv, .detailed.tsv, .report.out; with max_missing >= 0
// also .clean.tsv and .dropped.txt).  add(): one row, label and accession; add_rows_file(): the rows of a saved stdout, lines of fewer
// than four TAB-separated fields (banner, warnings) skipped.  A label without '_' makes write() end the run, naming it, before any file
// is made.  write() says on stderr how many accessions x loci it wrote.
struct AlleleCodes;
class AlleleTable {
  public:
    void add(const char *label, size_t label_len, const std::string &accession);
    void add(const std::string &label, const std::string &accession) { add(label.data(), label.size(), accession); }
    void add_rows_file(const std::string &path);
    void write(const std::string &prefix, long long max_missing) const;
    // the raw table as allele codes (dists.cpp); max_missing >= 0: only the accessions that write() puts into PREFIX.clean.tsv
    AlleleCodes codes(long long max_missing) const;
  private:
    struct Cell { std::string allele; size_t n = 0; };   // the first row's allele, the number of rows
    std::vector<std::string> accessions_;                // in order of their first row
    std::unordered_map<std::string, size_t> acc_index_;
    std::vector<std::map<std::string, Cell>> cells_;     // per accession: locus -> cell
    std::set<std::string> loci_;
    std::string bad_label_;
    bool bad_ = false;
};

// `search -s -m --alleles PREFIX --nearest`: per (locus, accession) the record of the locus with the largest share of its k-mers in the
// accession, and how many records the accession holds completely (cid_search_nearest_segments' cells, one group per run of records of a
// locus).  add_record(): every record of the scheme, in input order — its number is what a cell's `seg` is turned into.  merge_group():
// the cells of one group (n_colors of them, seg = the record's number in the batch + record_base) into the locus; a locus that recurs —
// a run cut by a batch boundary, a later run, another query file — is merged by merge(), the library's total order: the greater share
// wins, compared exactly, ties to the earlier record; n_perfect adds up.  write(): PREFIX.nearest.tsv, one line per accession (colour
// order) and locus (byte order) without a perfect record whose best share is at least min_share; a label without '_' ends the run as
// AlleleTable::write does.
class NearestTable {
  public:
    explicit NearestTable(size_t n_colors) : n_colors_(n_colors) {}
    static std::string locus_of(const std::string &label) { return label.substr(0, label.find('_')); }
    size_t n_records() const { return labels_.size(); }
    void add_record(const std::string &label);
    void merge_group(const std::string &locus, const cid_nearest *cells, size_t record_base);
    static void merge(cid_nearest &cell, const cid_nearest &later);
    void write(const std::string &prefix, const std::vector<std::string> &accessions, double min_share) const;
  private:
    size_t n_colors_;
    std::vector<std::string> labels_;                          // every record's label; a cell's seg is an index into it
    std::map<std::string, std::vector<cid_nearest>> loci_;     // locus -> one cell per accession
    std::string bad_label_;
    bool bad_ = false;
};

// ---------------------------------------------------------------- allele distances and clusters (dists.cpp)
// An accessions x loci table as u32 codes, what cid_dists_create takes: per locus the allele texts are numbered from 1 in order of first
// appearance, 0 = no call (NA or an empty cell).  Made from an AlleleTable in memory (AlleleTable::codes) or from a table file in the form
// of PREFIX.raw.tsv / PREFIX.clean.tsv (from_file: a missing header, a line with another number of cells — named by its number — and a
// repeated accession end the run; it touches no GPU).
// from_files (`dists --query`): the table's accessions, then the query file's, on the TABLE's loci in its order, the query's columns
// matched to them by name (a query locus the table lacks is ignored, a table locus the query lacks is no call for the query's accessions)
// and both files through one encoder.  No locus in common, a locus name repeated in either header and an accession in both files end
// the run with the file and the name; it touches no GPU either.
struct QueryAlign {
    std::string table, query;                                    // the two paths
    size_t n_table = 0;                                          // accessions [0, n_table) are the table's, the rest the query's
    size_t common = 0, only_table = 0, only_query = 0;           // loci
};
struct AlleleCodes {
    std::vector<std::string> accessions, loci;
    std::vector<uint32_t> codes;   // accessions x loci, row-major
    static AlleleCodes from_file(const std::string &path);
    static AlleleCodes from_files(const std::string &table, const std::string &query, QueryAlign &q);
};
// `dists`: PREFIX.dists.tsv and PREFIX.compared.tsv (A x A, one line per accession), written row block by row block from cid_dists_rows —
// the host never holds a whole matrix; with cluster also PREFIX.clusters.tsv: single linkage of the pairs with compared >= min_compared
// (at least 1) and differ <= threshold, and every accession's nearest comparable neighbour.  ctx is not used (may be null) for a table
// without accessions or without loci.  phase (may be null) is told when a part is done (COLORID_TIMING).  Says on stderr what it wrote.
// With mst, after all that, PREFIX.mst.tsv and PREFIX.mst.nwk: the minimum spanning forest (cid_dists_forest: the pairs with compared >=
// min_compared under the key differ, then more compared, then the earlier accessions) as an edge list in key order and as one Newick
// line per tree, rooted at the tree's first accession, children in table order, branch length = differ.  With no_matrices the two A x A
// files are not made: rows are fetched only for the clusters, and not at all without them.
// With within, after the matrices and before the clusters, PREFIX.within.tsv: a, b, differ, compared for every unordered pair with
// compared >= min_compared and differ <= within_threshold, a before b in the table, in order of (a's row, b's row), written block of
// rows by block of rows from cid_dists_within(CID_DISTS_UPPER): only those pairs leave the device.
// With closest = K (1 .. CID_DISTS_CLOSEST_MAX), after that, PREFIX.closest.tsv: accession, neighbour, differ, compared — the accessions
// in table order, under each its up to K nearest (cid_dists_closest: the others with compared >= min_compared and, with within,
// differ <= within_threshold; fewer differing loci first, then more shared loci, then table order), or one line of dashes.
// With hist, after that, PREFIX.hist.tsv: loci, differ_pairs, differ_cumulative, compared_pairs — one line per n = 0 .. L: the unordered
// pairs with compared >= min_compared and differ = n, their running sum, and the unordered pairs with compared = n
// (cid_dists_hist(CID_DISTS_UPPER) over all rows: 16 bytes a line leave the device).
// With levels (coarse to fine, 1 .. kDistsMaxLevels of them), before the forest's files, PREFIX.levels.tsv: accession, one column T<t> per
// level = the `cluster` column of PREFIX.clusters.tsv at threshold t, and address = those numbers joined by '.'; from the edges of the
// one cid_dists_forest call that mst takes its files from.
constexpr size_t kDistsMaxLevels = 32;
struct DistsOptions {
    bool cluster = false;
    uint64_t threshold = 0;      // --cluster T
    uint64_t min_compared = 1;   // --min-compared M (for --cluster, --mst and --within)
    bool mst = false;            // --mst
    bool no_matrices = false;    // --no-matrices (the caller refuses it without mst, cluster, within, closest, hist or levels)
    bool within = false;
    uint64_t within_threshold = 0;   // --within T
    uint32_t closest = 0;            // --closest K (0: not asked for)
    bool hist = false;               // --hist
    std::vector<uint64_t> levels;    // --levels T1,T2,..: descending, no value twice (empty: not asked for)
};
void dists_run(cid_ctx *ctx, const AlleleCodes &t, const std::string &prefix, const DistsOptions &opt, void (*phase)(const char *) = nullptr);
// `dists --query` (t, q from AlleleCodes::from_files; opt.within_threshold and opt.min_compared): PREFIX.query.tsv — query, neighbour, in
// (table / query), differ, compared: for every query accession in file order its neighbours among the table's and the other query
// accessions, nearest first (fewer differing loci, then more shared loci, then table before query, each in file order); one line of
// dashes for a query accession without a neighbour.  One device table of all accessions, cid_dists_within over the query's rows.  With
// opt.closest = K a query accession's list is its first K lines (cid_dists_closest over the query's rows instead), within the threshold
// when opt.within is set and whatever the distance when it is not.  ctx is not used (may be null) when the query has no accession.
// Says on stderr what it aligned, found and wrote.
void dists_query_run(cid_ctx *ctx, const AlleleCodes &t, const QueryAlign &q, const std::string &prefix, const DistsOptions &opt,
                     void (*phase)(const char *) = nullptr);

// ---------------------------------------------------------------- several GPUs (--gpus N / --devices a,b,..)
// When set, the drivers below shard every query over the group's ranks (cid_group_*); results are identical.
void set_group(cid_group *group, const std::vector<cid_index *> &replicas);
void set_stripes(cid_group *group, const std::vector<cid_index *> &stripes);   // the same calls over a colour-striped index

// ---------------------------------------------------------------- drivers (same names as the reference modules)
namespace perfect_search {
void batch_search(cid_ctx *, const std::vector<std::string> &files, const Bigsi &b);      // perfect_search.rs:6-60
// perfect_search.rs:62-120; alleles != nullptr (`--alleles`): every row printed is also added to the table; nearest != nullptr
// (`--nearest`, the batched route only): every batch goes through cid_search_nearest_segments as well
void batch_search_mf(cid_ctx *, const std::vector<std::string> &files, const Bigsi &b, AlleleTable *alleles = nullptr, NearestTable *nearest = nullptr);
}
namespace batch_search_pe {
// `search --gather PREFIX` (no reference counterpart): PREFIX.gather.tsv, the greedy cover of every query by accessions
// (cid_search_gather: what each accession ADDS to the ones listed before it).  One block per query: a row per round, then the
// `unexplained` line.  The file is made by open (and removed should the run die), appended to per query, whole after finish.
struct GatherOut {
    std::string path;
    FILE *f = nullptr;
    uint64_t min_new = 1000;
    size_t max_rows = 0;          // 0: the number of accessions
    size_t n_rounds = 0;
    double ms_calls = 0.0;
    void open(const std::string &prefix);
    // rows[n_rows] of the query's n_kmers distinct k-mers, n_hit of which have an accession at all
    void add(const std::string &query, const Bigsi &b, size_t n_kmers, const cid_gather_row *rows, size_t n_rows, uint64_t n_hit);
    void finish();
};
void batch_search(cid_ctx *, const std::vector<std::string> &files1, const std::vector<std::string> &files2, const Bigsi &b,
                  int64_t filter, double cov, bool gene_search, uint8_t qual_offset, GatherOut *gather = nullptr);     // batch_search_pe.rs:9-179
void batch_search_mf(cid_ctx *, const std::vector<std::string> &files, const Bigsi &b, double cov);   // -g -m: every FASTA record its own query
void batch_search_cover(cid_ctx *, const std::vector<std::string> &files, const Bigsi &b, double cov);   // -g -m --coverage: + where on the record
}
namespace read_id_mt_pe {
// block-gzip (BGZF) fastq input on one GPU takes the device front end (cid_fastq_*) unless COLORID_DEVICE_FASTQ=0
bool device_fastq_wanted(const std::vector<std::string> &fq, size_t n_files);
size_t device_fastq_stretch_bytes(size_t n_colors);   // text per stretch (n_colors == 0: before the index is known)
double device_fastq_host_share();                     // share of a stretch's text inflated by the reader's host threads
int device_fastq_host_threads(size_t n_files);
// read_id / batch_id --taxon TAXON [--exclude] (the reference's read_filter, src/read_filter.rs, fused into the classifying pass): the
// reads whose label — column 2 of their _reads.txt row — contains TAXON (--exclude: does not contain it) are written by the device
// front end as PREFIX_TAXON.fq.gz / PREFIX_TAXON_R1.fq.gz + _R2: the one-bin case of --split.
// --split (no reference counterpart; one read_filter pass per label there): EVERY read to the file of its label, decided by equality —
// bin c: accession c (one significant top hit), C: no_hits, C + 1: too_short, C + 2: no_significant_hits, C + 3: multiple_hits (a joined
// list of several top hits) — as PREFIX_<name>.fq.gz / _R1 + _R2 per non-empty bin (cid_fastq_split, once per file per step) and the
// manifest PREFIX_split.tsv.  Set before the streamers run.
struct ReadOutput {   // which reads the classifying pass writes as .fq.gz
    enum Mode { kNone, kTaxon, kSplit } mode = kNone;
    std::string taxon;         // kTaxon: --taxon TAXON
    bool exclude = false;      // kTaxon: --exclude
    bool gz_matches = false;   // --gz-matches: members with LZ77 matches
};
void set_read_output(const ReadOutput &o);
// --split, after the index is loaded and before a read is classified: the bins' file names (spaces and '/' become '_'); ends the run when
// two bins would share a file or when (C + 4) x n_files descriptors are more than the process may hold open
void split_prepare(const Bigsi &b, size_t n_files);
void per_read_stream_se(cid_ctx *, const std::vector<std::string> &fq, const Bigsi &b, size_t d, double fp_correct, size_t batch,
                        const std::string &prefix, uint8_t qual_offset, size_t start_sample);   // read_id_mt_pe.rs:835-951
void per_read_stream_pe(cid_ctx *, const std::vector<std::string> &fq, const Bigsi &b, size_t d, double fp_correct, size_t batch,
                        const std::string &prefix, uint8_t qual_offset, size_t start_sample);   // read_id_mt_pe.rs:701-832
void stream_fasta(cid_ctx *, const std::vector<std::string> &fq, const Bigsi &b, size_t d, double fp_correct, size_t batch,
                  const std::string &prefix, size_t start_sample);                              // read_id_mt_pe.rs:450-569
}

}  // namespace colorid
