// .bxi (bincode 1.x of BigsyMapNew, src/bigsi.rs:19-27 / SURVEY.md App. A) <-> device-resident index,
// and the index builder (src/build.rs:15-130) with the Bloom inserts done on the GPU.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <future>
#include <set>
#include <thread>

#include <fcntl.h>
#include <mutex>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../cid_host_math.hpp"
#include "../cid_records.hpp"
#include "colorid_host.hpp"

namespace colorid {

#define CID_TRY(expr)                                                  \
    do {                                                               \
        if ((expr) != CID_OK) die("%s: %s", #expr, cid_last_error()); \
    } while (0)

namespace {

struct BufReader {  // big sequential reads; the file is parsed once, front to back
    FILE *f;
    std::vector<uint8_t> buf;
    size_t pos = 0, end = 0;
    std::string label;   // non-empty: every error names the file (merge reads several)
    explicit BufReader(const std::string &path, bool name_in_errors = false)
        : f(fopen(path.c_str(), "rb")), buf(1u << 20), label(name_in_errors ? path : std::string()) {
        if (!f) die("Can't open index!: %s", path.c_str());
    }
    ~BufReader() { fclose(f); }
    [[noreturn]] void fail(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        char msg[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        if (label.empty()) die("%s", msg);
        die("%s: %s", label.c_str(), msg);
    }
    void need(size_t n) {
        if (end - pos >= n) return;
        memmove(buf.data(), buf.data() + pos, end - pos);
        end -= pos;
        pos = 0;
        if (n > buf.size()) buf.resize(n);
        while (end < n) {
            size_t got = fread(buf.data() + end, 1, buf.size() - end, f);
            if (got == 0) fail("can't deserialize: unexpected end of file");
            end += got;
        }
    }
    // bulk: what is buffered first, then straight from the file — large reads with several pread() threads (a copy out of the
    // page cache runs at one core's memory speed, ~10 GB/s; the upload that follows takes 50 GB/s)
    void read_exact(uint8_t *dst, size_t n) {
        if (n == 0) return;
        const size_t take = std::min(n, end - pos);
        memcpy(dst, buf.data() + pos, take);
        pos += take;
        size_t got = take;
        static const int n_threads = [] { const char *e = cli_env("COLORID_IO_THREADS"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : v; }();
        if (n - got >= (32u << 20) && n_threads > 1) {
            const off_t at = ftello(f);   // the FILE's logical position == the next byte this reader has not seen
            if (at >= 0) {
                const size_t rest = n - got, per = (rest + (size_t)n_threads - 1) / (size_t)n_threads;
                std::vector<int> bad((size_t)n_threads, 0);
                std::vector<std::thread> th;
                auto work = [&](int t) {
                    size_t o = (size_t)t * per;
                    const size_t stop = std::min(rest, o + per);
                    while (o < stop) {
                        const ssize_t g = pread(fileno(f), dst + got + o, stop - o, at + (off_t)o);
                        if (g <= 0) { bad[(size_t)t] = 1; return; }
                        o += (size_t)g;
                    }
                };
                for (int t = 1; t < n_threads; ++t) th.emplace_back(work, t);
                work(0);
                for (auto &x : th) x.join();
                for (int b : bad) if (b) fail("can't deserialize: unexpected end of file");
                if (fseeko(f, at + (off_t)rest, SEEK_SET) != 0) fail("can't deserialize: seek failed");
                return;
            }
        }
        while (got < n) {
            const size_t g = fread(dst + got, 1, n - got, f);
            if (g == 0) fail("can't deserialize: unexpected end of file");
            got += g;
        }
    }
    uint64_t tell() { return (uint64_t)ftello(f) - (end - pos); }   // the file offset of the next byte this reader hands out
    void seek(uint64_t at) {
        if (fseeko(f, (off_t)at, SEEK_SET) != 0) fail("can't deserialize: seek failed");
        pos = end = 0;
    }
    uint64_t u64() {
        need(8);
        uint64_t v;
        memcpy(&v, buf.data() + pos, 8);  // little-endian host
        pos += 8;
        return v;
    }
    std::string str() {
        const uint64_t n = u64();
        if (n > (1u << 30)) fail("can't deserialize: string of %llu bytes", (unsigned long long)n);
        need(n);
        std::string s(reinterpret_cast<const char *>(buf.data() + pos), n);
        pos += n;
        return s;
    }
};

void w64(FILE *f, uint64_t v) { fwrite(&v, 8, 1, f); }

// The index file mapped into memory before the GPU context exists (bigsi_read_ahead, called first thing by the subcommands that load
// an index): threads touch its pages — out of the page cache, or off the disk — while the runtime starts up (0.1-0.3 s), and the
// loader then hands the row records to cid_index_put_records straight from the mapping: no copy into a buffer of ours at all
// (fread's copy of a 2.8 GB file was most of the 0.15 s the load took).  COLORID_INDEX_MMAP=0 keeps the buffered reader.
struct MappedIndex {
    const uint8_t *p = nullptr;
    size_t n = 0;
};
std::mutex g_map_mu;
std::map<std::string, MappedIndex> g_mapped;

}  // namespace

void bigsi_read_ahead(const std::string &path) {
    if (const char *e = cli_env("COLORID_INDEX_MMAP")) if (atoi(e) == 0) return;
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;   // (the loader reports it)
    struct stat st;
    // small files: nothing to gain; files beyond 64 GiB (a striped index of several GPUs' worth) stay with the sequential buffered
    // reader: four threads touching such a file ahead of the loader would fight it for the disk and the page cache
    if (fstat(fd, &st) != 0 || st.st_size < (off_t)(64 << 20) || st.st_size > (off_t)(64ll << 30)) { close(fd); return; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return;
    (void)madvise(m, (size_t)st.st_size, MADV_WILLNEED);
    MappedIndex mi;
    mi.p = static_cast<const uint8_t *>(m);
    mi.n = (size_t)st.st_size;
    {
        std::lock_guard<std::mutex> lk(g_map_mu);
        g_mapped[path] = mi;
    }
    const int n_threads = 4;
    for (int t = 0; t < n_threads; ++t)
        std::thread([mi, t, n_threads] {   // page tables filled in ahead of the upload (detached: the process outlives them or exits)
            const size_t per = (mi.n + (size_t)n_threads - 1) / (size_t)n_threads, lo = (size_t)t * per, hi = std::min(mi.n, lo + per);
            for (size_t o = lo; o < hi; o += 4096) (void)*(volatile const uint8_t *)(mi.p + o);
        }).detach();
}

namespace {
MappedIndex mapped_index(const std::string &path) {
    std::lock_guard<std::mutex> lk(g_map_mu);
    auto it = g_mapped.find(path);
    return it == g_mapped.end() ? MappedIndex() : it->second;
}
}  // namespace

namespace {

// The file up to its row records: the struct's scalars, then the colours by id.  Returns the number of row records; r is left at
// the first of them.
uint64_t read_header(BufReader &r, const std::string &path, Bigsi &b) {
    b.bloom_size = r.u64();
    b.num_hash = r.u64();
    b.k_size = r.u64();
    const bool mini = path.size() >= 4 && path.compare(path.size() - 4, 4, ".mxi") == 0;   // the suffix selects the struct (main.rs:723)
    if (mini) b.m_size = r.u64();                                                            // BigsyMapMiniNew.m_size
    const uint64_t nc = r.u64();
    if (nc == 0 || nc > (1u << 24)) r.fail("can't deserialize: %llu colours", (unsigned long long)nc);
    b.colors.assign(nc, std::string());
    for (uint64_t i = 0; i < nc; ++i) {
        const uint64_t id = r.u64();
        std::string name = r.str();
        if (id >= nc) r.fail("can't deserialize: colour id %llu of %llu", (unsigned long long)id, (unsigned long long)nc);
        b.colors[id] = std::move(name);
    }
    return r.u64();
}

size_t record_bytes(const Bigsi &b) { return cid::record_bytes(b.colors.size()); }

// The file after its row records: n_ref_kmers by accession name, kept in colour order
void read_tail(BufReader &r, Bigsi &b) {
    const uint64_t nc = b.colors.size();
    b.n_ref_kmers.assign(nc, 0);
    std::map<std::string, uint64_t> by_name;
    for (uint64_t c = 0; c < nc; ++c) by_name[b.colors[c]] = c;
    const uint64_t n_ref = r.u64();
    for (uint64_t i = 0; i < n_ref; ++i) {
        std::string name = r.str();
        const uint64_t v = r.u64();
        auto it = by_name.find(name);
        if (it != by_name.end()) b.n_ref_kmers[it->second] = v;
    }
}

// The row records go to the device as they sit in the file — { u64 row ; u64 W32 ; W32 x u32 ; u64 nbits } each — and are parsed and
// checked there (put: cid_index_put_records or one of its kin): straight from the mapping when bigsi_read_ahead made one, else a second
// thread reads the next chunk while this one is uploaded.  r is at the first record and is left just past the last.
void stream_records(BufReader &r, const std::string &path, uint64_t n_rows, size_t rec, const std::function<int(const uint8_t *, size_t)> &put) {
    if (const MappedIndex mi = mapped_index(path); mi.p) {
        const uint64_t at = r.tell();
        if (at > mi.n || n_rows * rec > mi.n - at) die("can't deserialize: unexpected end of file");
        const size_t chunk_recs = std::max<size_t>(1, (256u << 20) / rec);
        for (uint64_t done = 0; done < n_rows;) {
            const size_t nr = (size_t)std::min<uint64_t>(n_rows - done, chunk_recs);
            const int rc = put(mi.p + at + done * rec, nr);
            if (rc != CID_OK) die("can't deserialize: %s", cid_last_error());
            done += nr;
        }
        r.seek(at + n_rows * rec);
    } else {
        const size_t chunk_recs = std::max<size_t>(1, (128u << 20) / rec);
        std::vector<uint8_t> bufs[2];
        size_t have[2] = {0, 0};
        uint64_t left = n_rows;
        auto fill = [&](int which) {
            const size_t nr = (size_t)std::min<uint64_t>(left, chunk_recs);
            bufs[which].resize(nr * rec);
            r.read_exact(bufs[which].data(), nr * rec);
            have[which] = nr;
            left -= nr;
        };
        fill(0);
        int cur = 0;
        while (have[cur]) {
            std::thread prefetch([&, cur] { fill(cur ^ 1); });
            const int rc = put(bufs[cur].data(), have[cur]);
            prefetch.join();
            if (rc != CID_OK) die("can't deserialize: %s", cid_last_error());
            cur ^= 1;
        }
    }
}

}  // namespace

Bigsi read_bigsi(cid_ctx *ctx, const std::string &path, int hash_variant, bool meta_only, cid_group *group, std::vector<cid_index *> *stripes) {
    BufReader r(path);
    Bigsi b;
    const uint64_t n_rows = read_header(r, path, b);
    const bool mini = b.m_size != 0;
    const uint64_t nc = b.colors.size();
    const uint32_t w32 = (uint32_t)((nc + 31) / 32);
    if (!meta_only && stripes) {   // one colour stripe per rank of the group (an index larger than one GPU's HBM)
        if (mini) die("Error: an index with minimizers (.mxi) cannot be striped over GPUs");
        int n_ranks = 0;
        CID_TRY(cid_group_size(group, &n_ranks));
        stripes->assign((size_t)n_ranks, nullptr);
        CID_TRY(cid_group_stripes_create(group, b.bloom_size, (uint32_t)b.num_hash, (uint32_t)b.k_size, (uint32_t)nc, hash_variant, stripes->data()));
    } else if (!meta_only) {
        CID_TRY(cid_index_create(ctx, b.bloom_size, (uint32_t)b.num_hash, (uint32_t)b.k_size, (uint32_t)nc, hash_variant, &b.index));
        if (mini) CID_TRY(cid_index_set_minimizer(b.index, (uint32_t)b.m_size));
    }
    const size_t rec = record_bytes(b);
    if (n_rows > (~0ull) / rec) die("can't deserialize: %llu rows", (unsigned long long)n_rows);
    if (meta_only) {   // `info`: no device; the records are still checked, as deserialising them would
        std::vector<uint8_t> chunk;
        for (uint64_t left = n_rows; left;) {
            const size_t nr = (size_t)std::min<uint64_t>(left, (16u << 20) / rec + 1);
            chunk.resize(nr * rec);
            r.read_exact(chunk.data(), nr * rec);
            for (size_t i = 0; i < nr; ++i) {
                uint64_t nw, nbits;
                memcpy(&nw, chunk.data() + i * rec + 8, 8);
                memcpy(&nbits, chunk.data() + i * rec + 16 + 4ull * w32, 8);
                if (nw != w32) die("can't deserialize: row with %llu words, expected %u", (unsigned long long)nw, w32);
                if (nbits != nc) die("can't deserialize: row of %llu bits, expected %llu", (unsigned long long)nbits, (unsigned long long)nc);
            }
            left -= nr;
        }
    } else {
        stream_records(r, path, n_rows, rec, [&](const uint8_t *src, size_t nr) {
            return stripes ? cid_group_stripes_put_records(group, stripes->data(), src, nr) : cid_index_put_records(b.index, src, nr);
        });
    }
    read_tail(r, b);
    if (!meta_only && stripes) {
        for (cid_index *ix : *stripes) CID_TRY(cid_index_finalize(ix));
    } else if (!meta_only) CID_TRY(cid_index_finalize(b.index));
    return b;
}

namespace {

// What `merge`, `subset`, `compare`, `fold` and `collapse` (cmd) have in common: the input index of a command that streams row records.  Its checks read only
// the header and the n_ref_kmers tail (the tail lies at header_end + n_rows x record_bytes), so a refusal costs no GPU context and no
// pass over the rows.
bool is_mxi(const std::string &p) { return p.size() >= 4 && p.compare(p.size() - 4, 4, ".mxi") == 0; }

// The input exists and is not the file the command is about to write (out_path; `instead`: what to write elsewhere; null: the command
// writes no index).  Returns the input's size in bytes.
uint64_t stat_input(const char *cmd, const std::string &path, const std::string *out_path = nullptr, const char *instead = nullptr) {
    struct stat st, out_st;
    if (stat(path.c_str(), &st) != 0) die("Can't open index!: %s", path.c_str());
    if (out_path && stat(out_path->c_str(), &out_st) == 0 && st.st_dev == out_st.st_dev && st.st_ino == out_st.st_ino)
        die("%s: the output %s is the input %s: write the %s to another file", cmd, out_path->c_str(), path.c_str(), instead);
    return (uint64_t)st.st_size;
}

// in.path's header and n_ref_kmers tail into in.meta, its number of row records into in.n_rows; the records and the count of the tail
// must fit in the file's file_size bytes
void read_input_meta(const char *cmd, IndexInput &in, uint64_t file_size) {
    BufReader r(in.path, /*name_in_errors=*/true);
    in.n_rows = read_header(r, in.path, in.meta);
    const uint64_t header_end = r.tell();
    const size_t rec = record_bytes(in.meta);
    if (in.n_rows > file_size / rec || header_end + in.n_rows * rec + 8 > file_size)
        die("%s: %s is truncated: %llu row records of %zu bytes from byte %llu do not fit in its %llu bytes", cmd, in.path.c_str(),
            (unsigned long long)in.n_rows, rec, (unsigned long long)header_end, (unsigned long long)file_size);
    r.seek(header_end + in.n_rows * rec);
    read_tail(r, in.meta);
}

// The checked input's row records to `put`: the file is opened again and must still be what read_input_meta saw (how: "merged" / "read")
void stream_input(const char *cmd, const char *how, const IndexInput &in, const std::function<int(const uint8_t *, size_t)> &put) {
    BufReader r(in.path, /*name_in_errors=*/true);
    Bigsi again;
    if (read_header(r, in.path, again) != in.n_rows || again.colors != in.meta.colors) die("%s: %s changed while it was %s", cmd, in.path.c_str(), how);
    stream_records(r, in.path, in.n_rows, record_bytes(in.meta), put);
}

// the index a command writes, made on ctx from its metadata: empty, not finalized
void create_output_index(cid_ctx *ctx, Bigsi &out) {
    CID_TRY(cid_index_create(ctx, out.bloom_size, (uint32_t)out.num_hash, (uint32_t)out.k_size, (uint32_t)out.colors.size(), CID_HASH_XXH3_V08, &out.index));
    if (out.m_size) CID_TRY(cid_index_set_minimizer(out.index, (uint32_t)out.m_size));
}

// build numbers colours in name order (build.rs:105); colour c must not sort before colour c - 1
void check_name_order_at(const char *cmd, const std::string &path, const std::vector<std::string> &colors, uint64_t c) {
    if (c && colors[c] < colors[c - 1])
        die("%s: %s numbers its accessions out of name order (%s before %s): %s takes indices as build writes them", cmd, path.c_str(),
            colors[c - 1].c_str(), colors[c].c_str(), cmd);
}

[[noreturn]] void die_accession_twice(const char *cmd, const std::string &path, const std::string &name) {
    die("%s: %s holds accession %s twice", cmd, path.c_str(), name.c_str());
}

}  // namespace

// merge: no counterpart in the reference.
Bigsi merge_check(const std::vector<std::string> &paths, const std::string &out_path, std::vector<MergeInput> &inputs) {
    if (paths.size() < 2) die("merge needs at least two input indices (-i a.bxi b.bxi ...), got %zu", paths.size());
    for (const std::string &p : paths)
        if (is_mxi(p) != is_mxi(paths[0]))
            die("merge: %s and %s are not the same kind of index (.bxi / .mxi): inputs must all be .bxi or all .mxi", paths[0].c_str(), p.c_str());
    inputs.assign(paths.size(), MergeInput());
    std::map<std::string, std::pair<size_t, uint64_t>> owner;   // accession -> (input, colour in it); iterates in byte order, as tab_to_map
    uint64_t total = 0;
    for (size_t i = 0; i < paths.size(); ++i) {
        MergeInput &in = inputs[i];
        in.path = paths[i];
        read_input_meta("merge", in, stat_input("merge", in.path, &out_path, "merged index"));
        const Bigsi &a = inputs[0].meta, &b = in.meta;
        const struct { const char *name; uint64_t first, here; } fields[] = {
            {"bloom_size", a.bloom_size, b.bloom_size}, {"num_hash", a.num_hash, b.num_hash}, {"k_size", a.k_size, b.k_size}, {"m_size", a.m_size, b.m_size}};
        for (const auto &f : fields)
            if (f.first != f.here)
                die("merge: %s differs: %llu in %s, %llu in %s", f.name, (unsigned long long)f.first, inputs[0].path.c_str(), (unsigned long long)f.here,
                    in.path.c_str());
        for (uint64_t c = 0; c < b.colors.size(); ++c) {
            check_name_order_at("merge", in.path, b.colors, c);   // the deposit needs that order (an increasing colour map)
            const auto ins = owner.emplace(b.colors[c], std::make_pair(i, c));
            if (!ins.second) {
                const size_t j = ins.first->second.first;
                if (j == i) die_accession_twice("merge", in.path, b.colors[c]);
                die("merge: accession %s is in both %s and %s", b.colors[c].c_str(), inputs[j].path.c_str(), in.path.c_str());
            }
        }
        total += b.colors.size();
    }
    if (total > (1u << 20)) die("merge: %llu accessions in all, more than an index holds (2^20 = 1048576)", (unsigned long long)total);
    Bigsi m;
    m.bloom_size = inputs[0].meta.bloom_size; m.num_hash = inputs[0].meta.num_hash; m.k_size = inputs[0].meta.k_size; m.m_size = inputs[0].meta.m_size;
    for (MergeInput &in : inputs) in.colour_map.assign(in.meta.colors.size(), 0);
    for (const auto &kv : owner) {
        MergeInput &in = inputs[kv.second.first];
        in.colour_map[kv.second.second] = (uint32_t)m.colors.size();
        m.colors.push_back(kv.first);
        m.n_ref_kmers.push_back(in.meta.n_ref_kmers[kv.second.second]);
    }
    return m;
}

void merge_records(cid_ctx *ctx, Bigsi &m, const std::vector<MergeInput> &inputs) {
    create_output_index(ctx, m);
    for (size_t i = 0; i < inputs.size(); ++i) {
        const MergeInput &in = inputs[i];
        fprintf(stderr, "Merging %s into index (%zu/%zu): %zu accessions, %llu rows\n", in.path.c_str(), i + 1, inputs.size(), in.meta.colors.size(),
                (unsigned long long)in.n_rows);
        stream_input("merge", "merged", in, [&](const uint8_t *src, size_t nr) {
            return cid_index_put_records_mapped(m.index, src, nr, (uint32_t)in.meta.colors.size(), in.colour_map.data());
        });
    }
}

// subset: no counterpart in the reference.  Beside the input's own checks, every refusal comes from the list.
Bigsi subset_check(const std::string &in_path, const std::string &out_path, const std::string &list_path, bool exclude, SubsetInput &in) {
    in.path = in_path;
    const uint64_t file_size = stat_input("subset", in.path, &out_path, "subset");
    // the list: the text before the first TAB of every non-empty line (a `build -r` reference list is one); a repeated name counts once
    std::set<std::string> listed;
    {
        FILE *f = fopen(list_path.c_str(), "rb");
        if (!f) die("subset: can't open the accession list %s", list_path.c_str());
        std::string text;
        char buf[1 << 16];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
        fclose(f);
        for (size_t p = 0; p < text.size();) {
            size_t e = text.find('\n', p);
            if (e == std::string::npos) e = text.size();
            std::string line = text.substr(p, e - p);
            p = e + 1;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            listed.insert(line.substr(0, line.find('\t')));
        }
    }
    if (listed.empty()) die("subset: the accession list %s is empty", list_path.c_str());
    read_input_meta("subset", in, file_size);
    const Bigsi &a = in.meta;
    std::map<std::string, uint64_t> colour_of;
    for (uint64_t c = 0; c < a.colors.size(); ++c) {
        check_name_order_at("subset", in.path, a.colors, c);   // the kept colours keep their order, and build's order is name order
        if (!colour_of.emplace(a.colors[c], c).second) die_accession_twice("subset", in.path, a.colors[c]);
    }
    for (const std::string &name : listed)
        if (!colour_of.count(name))
            die("subset: accession %s of %s is not in %s", name.c_str(), list_path.c_str(), in.path.c_str());
    Bigsi out;
    out.bloom_size = a.bloom_size; out.num_hash = a.num_hash; out.k_size = a.k_size; out.m_size = a.m_size;
    in.keep_words.assign((a.colors.size() + 31) / 32, 0u);
    for (uint64_t c = 0; c < a.colors.size(); ++c)
        if ((listed.count(a.colors[c]) != 0) != exclude) {
            in.keep_words[c / 32] |= 1u << (c % 32);
            out.colors.push_back(a.colors[c]);
            out.n_ref_kmers.push_back(a.n_ref_kmers[c]);
        }
    if (out.colors.empty())
        die("subset: nothing left to keep: %s excludes all %zu accessions of %s", list_path.c_str(), a.colors.size(), in.path.c_str());
    if (out.colors.size() > (1u << 20))
        die("subset: %zu accessions kept from %s, more than an index holds (2^20 = 1048576)", out.colors.size(), in.path.c_str());
    return out;
}

void subset_records(cid_ctx *ctx, Bigsi &out, const SubsetInput &in) {
    create_output_index(ctx, out);
    fprintf(stderr, "Extracting %zu of %zu accessions from %s: %llu rows\n", out.colors.size(), in.meta.colors.size(), in.path.c_str(),
            (unsigned long long)in.n_rows);
    stream_input("subset", "read", in, [&](const uint8_t *src, size_t nr) {
        return cid_index_put_records_subset(out.index, src, nr, (uint32_t)in.meta.colors.size(), in.keep_words.data());
    });
}

// collapse: no counterpart in the reference.  Beside the input's own checks, every refusal comes from the groups file.
Bigsi collapse_check(const std::string &in_path, const std::string &out_path, const std::string &groups_path, CollapseInput &in) {
    in.path = in_path;
    const uint64_t file_size = stat_input("collapse", in.path, &out_path, "collapsed index");
    // the groups file: `accession TAB group` on every non-empty line; what follows a second TAB is ignored
    std::map<std::string, std::string> group_of_name;
    {
        FILE *f = fopen(groups_path.c_str(), "rb");
        if (!f) die("collapse: can't open the groups file %s", groups_path.c_str());
        std::string text;
        char buf[1 << 16];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
        fclose(f);
        uint64_t line_no = 0;
        for (size_t p = 0; p < text.size();) {
            size_t e = text.find('\n', p);
            if (e == std::string::npos) e = text.size();
            std::string line = text.substr(p, e - p);
            p = e + 1;
            ++line_no;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            const size_t t1 = line.find('\t');
            if (t1 == std::string::npos)
                die("collapse: line %llu of %s has no TAB ('%s'): expected accession TAB group", (unsigned long long)line_no, groups_path.c_str(), line.c_str());
            const size_t t2 = line.find('\t', t1 + 1);
            const std::string acc = line.substr(0, t1), group = line.substr(t1 + 1, t2 == std::string::npos ? std::string::npos : t2 - t1 - 1);
            if (acc.empty()) die("collapse: line %llu of %s has an empty accession name (group %s)", (unsigned long long)line_no, groups_path.c_str(), group.c_str());
            if (group.empty()) die("collapse: line %llu of %s has an empty group name (accession %s)", (unsigned long long)line_no, groups_path.c_str(), acc.c_str());
            if (!group_of_name.emplace(acc, group).second) die("collapse: %s lists accession %s twice", groups_path.c_str(), acc.c_str());
        }
    }
    read_input_meta("collapse", in, file_size);
    const Bigsi &a = in.meta;
    if (a.colors.size() > (1u << 20))
        die("collapse: %s holds %zu accessions, more than an index holds (2^20 = 1048576)", in.path.c_str(), a.colors.size());
    std::map<std::string, uint32_t> colour_of;
    for (uint32_t c = 0; c < a.colors.size(); ++c)
        if (!colour_of.emplace(a.colors[c], c).second) die_accession_twice("collapse", in.path, a.colors[c]);
    for (const auto &kv : group_of_name)
        if (!colour_of.count(kv.first)) die("collapse: accession %s of %s is not in %s", kv.first.c_str(), groups_path.c_str(), in.path.c_str());
    // a group may carry an accession's name only when the file puts that accession into it: two colours must not end under one name
    for (const auto &kv : group_of_name) {
        if (!colour_of.count(kv.second)) continue;
        const auto own = group_of_name.find(kv.second);
        if (own == group_of_name.end() || own->second != kv.second)
            die("collapse: group %s of %s (accession %s) carries the name of accession %s of %s, which is not a member of it", kv.second.c_str(),
                groups_path.c_str(), kv.first.c_str(), kv.second.c_str(), in.path.c_str());
    }
    std::map<std::string, std::vector<uint32_t>> groups;   // iterates in byte order, as tab_to_map: build's colour numbering
    for (uint32_t c = 0; c < a.colors.size(); ++c) {
        const auto it = group_of_name.find(a.colors[c]);
        groups[it == group_of_name.end() ? a.colors[c] : it->second].push_back(c);
    }
    Bigsi out;
    out.bloom_size = a.bloom_size; out.num_hash = a.num_hash; out.k_size = a.k_size; out.m_size = a.m_size;
    in.group_of.assign(a.colors.size(), 0u);
    for (auto &kv : groups) {
        for (const uint32_t c : kv.second) in.group_of[c] = (uint32_t)out.colors.size();
        out.colors.push_back(kv.first);
        in.members.push_back(std::move(kv.second));
    }
    out.n_ref_kmers.assign(out.colors.size(), 0);
    return out;
}

uint64_t collapse_n_ref(uint64_t bloom_size, uint64_t num_hash, const std::vector<uint64_t> &n_i, const std::vector<uint64_t> &bits_i,
                        uint64_t bits_group) {
    if (n_i.size() == 1) return n_i[0];
    uint64_t sum = 0, most = 0;
    bool full = bits_group >= bloom_size;
    for (size_t i = 0; i < n_i.size(); ++i) {
        if (n_i[i] == 0) return 0;
        sum += n_i[i];
        most = std::max(most, n_i[i]);
        full = full || bits_i[i] >= bloom_size;
    }
    if (full) return sum;
    const double m = (double)bloom_size, n = (double)num_hash;
    auto est = [&](uint64_t x) { return -(m / n) * std::log1p(-(double)x / m); };
    double members = 0.0;
    for (const uint64_t x : bits_i) members += est(x);
    if (!(members > 0.0)) return sum;   // empty columns: nothing to estimate from
    const double v = std::floor((double)sum * est(bits_group) / members + 0.5);
    return v <= (double)most ? most : v >= (double)sum ? sum : (uint64_t)v;
}

void collapse_records(cid_ctx *ctx, Bigsi &out, CollapseInput &in) {
    create_output_index(ctx, out);
    const Bigsi &a = in.meta;
    fprintf(stderr, "Collapsing %zu accessions of %s into %zu groups\n", a.colors.size(), in.path.c_str(), out.colors.size());
    in.bits_file.assign(a.colors.size(), 0);
    in.bits_index.assign(out.colors.size(), 0);
    stream_input("collapse", "read", in, [&](const uint8_t *src, size_t nr) {
        return cid_index_put_records_grouped(out.index, src, nr, (uint32_t)a.colors.size(), in.group_of.data(), in.bits_file.data(),
                                             in.bits_index.data());
    });
    for (size_t g = 0; g < out.colors.size(); ++g) {
        std::vector<uint64_t> n_i, bits_i;
        for (const uint32_t c : in.members[g]) { n_i.push_back(a.n_ref_kmers[c]); bits_i.push_back(in.bits_file[c]); }
        out.n_ref_kmers[g] = collapse_n_ref(a.bloom_size, a.num_hash, n_i, bits_i, in.bits_index[g]);
    }
}

// fold: no counterpart in the reference.  Beside the input's own checks, every refusal comes from the requested size.
Bigsi fold_check(const std::string &in_path, const std::string &out_path, char by, const std::string &value, FoldInput &in) {
    in.path = in_path;
    read_input_meta("fold", in, stat_input("fold", in.path, &out_path, "folded index"));
    const Bigsi &a = in.meta;
    const uint64_t m = a.bloom_size;
    if (m == 0) die("fold: %s states a Bloom size of 0", in.path.c_str());
    auto worst_at = [&](uint64_t size, size_t &worst) {   // the highest false_prob over the accessions at `size` rows (the first of equals)
        double fp = -1.0;
        for (size_t c = 0; c < a.colors.size(); ++c) {
            const double v = false_prob((double)size, (double)a.num_hash, (double)a.n_ref_kmers[c]);
            if (v > fp) { fp = v; worst = c; }
        }
        return fp;
    };
    uint64_t new_size = 0;
    char *end = nullptr;
    if (by == 'p') {
        const double bound = strtod(value.c_str(), &end);
        if (value.empty() || *end || !(bound > 0.0 && bound < 1.0))
            die("fold: -p %s: the false-positive bound must be a number above 0 and below 1", value.c_str());
        size_t worst = 0;
        const double own = worst_at(m, worst);
        if (!(own <= bound))
            die("fold: -p %s: %s misses the bound at its own size %llu already: accession %s (%llu k-mers) predicts %.6g; nothing to fold",
                value.c_str(), in.path.c_str(), (unsigned long long)m, a.colors[worst].c_str(), (unsigned long long)a.n_ref_kmers[worst], own);
        const size_t heavy = worst;   // most sizes fail on the accession that is worst at the input's size: ask it first
        for (const uint64_t d : cid::divisors_of(m)) {   // ascending: the first that holds every accession under the bound
            if (!(false_prob((double)d, (double)a.num_hash, (double)a.n_ref_kmers[heavy]) <= bound)) continue;
            if (worst_at(d, worst) <= bound) { new_size = d; break; }
        }
    } else {
        errno = 0;
        const unsigned long long v = strtoull(value.c_str(), &end, 10);
        if (value.empty() || value[0] < '0' || value[0] > '9' || *end || (v == ~0ull && errno == ERANGE))
            die("fold: -%c %s: expected a whole number", by, value.c_str());
        if (by == 's') {
            if (v == 0 || v > m)
                die("fold: -s %llu: the new Bloom size must be between 1 and the %llu of %s", v, (unsigned long long)m, in.path.c_str());
            if (cid::fold_factor(m, v) == 0) {
                uint64_t below, above;
                cid::nearest_divisors(m, v, below, above);
                die("fold: -s %llu does not divide the Bloom size %llu of %s: the nearest sizes that do are %llu and %llu", v, (unsigned long long)m,
                    in.path.c_str(), (unsigned long long)below, (unsigned long long)above);
            }
            new_size = v;
        } else {
            if (cid::fold_factor(m, v) == 0)
                die("fold: -f %llu: the factor must be a divisor of the Bloom size %llu of %s", v, (unsigned long long)m, in.path.c_str());
            new_size = m / v;
        }
    }
    in.factor = m / new_size;
    in.worst_fp = worst_at(new_size, in.worst);
    Bigsi out;
    out.bloom_size = new_size; out.num_hash = a.num_hash; out.k_size = a.k_size; out.m_size = a.m_size;
    out.colors = a.colors;
    out.n_ref_kmers = a.n_ref_kmers;
    if (out.colors.size() > (1u << 20))
        die("fold: %s holds %zu accessions, more than an index holds (2^20 = 1048576)", in.path.c_str(), out.colors.size());
    return out;
}

void fold_records(cid_ctx *ctx, Bigsi &out, const FoldInput &in) {
    create_output_index(ctx, out);
    fprintf(stderr, "Folding %s: %llu rows into %llu\n", in.path.c_str(), (unsigned long long)in.n_rows, (unsigned long long)out.bloom_size);
    stream_input("fold", "read", in, [&](const uint8_t *src, size_t nr) {
        return cid_index_put_records_folded(out.index, src, nr, in.meta.bloom_size);
    });
}

// compare: no counterpart in the reference.  Every refusal but one comes from the input's own checks.
void compare_check(const std::string &in_path, CompareInput &in) {
    in.path = in_path;
    read_input_meta("compare", in, stat_input("compare", in.path));
    std::set<std::string> seen;
    for (const std::string &name : in.meta.colors)
        if (!seen.insert(name).second) die_accession_twice("compare", in.path, name);
    if (in.meta.colors.size() > (1u << 20))
        die("compare: %s holds %zu accessions, more than the pair counters take (2^20 = 1048576)", in.path.c_str(), in.meta.colors.size());
}

// the one refusal that needs the device: counters that do not fit in its memory (cid_pairs_create says how many bytes)
std::vector<uint64_t> compare_records(cid_ctx *ctx, const CompareInput &in) {
    const size_t nc = in.meta.colors.size();
    cid_pairs *pairs = nullptr;
    if (cid_pairs_create(ctx, in.meta.bloom_size, (uint32_t)nc, &pairs) != CID_OK) die("compare: %s: %s", in.path.c_str(), cid_last_error());
    fprintf(stderr, "Comparing %zu accessions of %s: %llu rows\n", nc, in.path.c_str(), (unsigned long long)in.n_rows);
    stream_input("compare", "read", in, [&](const uint8_t *src, size_t nr) { return cid_pairs_add_records(pairs, src, nr); });
    std::vector<uint64_t> shared(nc * nc);
    CID_TRY(cid_pairs_fetch(pairs, shared.data()));
    cid_pairs_destroy(pairs);
    return shared;
}

void save_bigsi(const std::string &path, const Bigsi &b) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("problems preparing serialized data for writing: %s", path.c_str());
    const uint64_t nc = b.colors.size();
    const uint32_t w32 = (uint32_t)((nc + 31) / 32);
    w64(f, b.bloom_size); w64(f, b.num_hash); w64(f, b.k_size);
    if (b.m_size) w64(f, b.m_size);
    w64(f, nc);
    for (uint64_t c = 0; c < nc; ++c) { w64(f, c); w64(f, b.colors[c].size()); fwrite(b.colors[c].data(), 1, b.colors[c].size(), f); }
    // rows come back from the device in ascending order; all-zero rows are dropped (build.rs:123-127)
    const long count_pos = ftell(f);
    w64(f, 0);
    uint64_t n_rows = 0;
    const size_t rec = 24 + 4ull * w32;
    const uint64_t chunk = std::max<uint64_t>(1, (128u << 20) / rec);   // records are formatted on the device; the host writes bytes
    std::vector<uint8_t> records(chunk * rec);
    for (uint64_t r0 = 0; r0 < b.bloom_size; r0 += chunk) {
        const uint64_t nr = std::min<uint64_t>(chunk, b.bloom_size - r0);
        uint64_t got = 0;
        CID_TRY(cid_index_get_records(b.index, r0, nr, records.data(), &got));
        if (got && fwrite(records.data(), rec, got, f) != got) die("problems writing %s", path.c_str());
        n_rows += got;
    }
    w64(f, nc);
    for (uint64_t c = 0; c < nc; ++c) { w64(f, b.colors[c].size()); fwrite(b.colors[c].data(), 1, b.colors[c].size(), f); w64(f, b.n_ref_kmers[c]); }
    fseek(f, count_pos, SEEK_SET);
    w64(f, n_rows);
    fclose(f);
}

// tab_to_map (build.rs:15-31): accession \t file [\t file2]; later lines overwrite earlier ones
std::map<std::string, std::vector<std::string>> tab_to_map(const std::string &ref_tsv) {
    std::map<std::string, std::vector<std::string>> refs;  // std::map iterates sorted == accessions.sort() (build.rs:105)
    LineReader r(ref_tsv);
    std::string line;
    while (r.next(line)) {
        std::vector<std::string> v;
        size_t p = 0;
        while (true) {
            size_t e = line.find('\t', p);
            v.push_back(line.substr(p, e == std::string::npos ? std::string::npos : e - p));
            if (e == std::string::npos) break;
            p = e + 1;
        }
        if (v.size() < 2) die("reference file line without a tab: '%s'", line.c_str());
        refs[v[0]] = v.size() == 2 ? std::vector<std::string>{v[1]} : std::vector<std::string>{v[1], v[2]};
    }
    return refs;
}

size_t hashcheck(cid_ctx *ctx, Bigsi &b, const std::string &ref_tsv, uint8_t quality, const char *const *variant_names, std::vector<double> &worst) {
    if (b.m_size) die("hashcheck works on k-mer indices (.bxi); a minimizer index shares its hash with the .bxi built by the same binary");
    const auto refs = tab_to_map(ref_tsv);
    const size_t C = b.colors.size();
    std::vector<uint64_t> hits(C);
    size_t n_checked = 0;
    printf("variant\taccession\tkmers\tpresent\tfraction\n");
    for (auto &kv : refs) {
        const auto it = std::find(b.colors.begin(), b.colors.end(), kv.first);
        if (it == b.colors.end()) { fprintf(stderr, "%s is not an accession of the index: skipped\n", kv.first.c_str()); continue; }
        const uint32_t colour = (uint32_t)(it - b.colors.begin());
        const std::vector<std::string> &v = kv.second;
        const bool is_gz = v.size() == 2 || (v[0].size() >= 2 && v[0].compare(v[0].size() - 2, 2, "gz") == 0);
        // the accession's k-mers as build counts them (reads: with the automatic cutoff, the build default)
        cid_kmerset *ks = nullptr;
        KmerMap km((uint32_t)b.k_size);
        uint64_t nk = 0;
        if (gpu_counting_enabled(b.k_size))
            ks = is_gz ? count_fastq_gpu(ctx, b.k_size, v[0], v.size() == 2 ? &v[1] : nullptr, quality) : count_fasta_gpu(ctx, b.k_size, read_fasta(v[0]));
        if (ks) {
            if (is_gz) { const int64_t t = auto_cutoff_gpu(ks); CID_TRY(cid_kmerset_clean(ks, (uint64_t)(t < 0 ? 0 : t))); }
            CID_TRY(cid_kmerset_size(ks, &nk));
        } else {
            if (v.size() == 2) kmers_fq_pe_qual(v[0], v[1], quality, km);
            else if (is_gz) kmers_from_fq_qual(v[0], quality, km);
            else kmerize_vector(read_fasta(v[0]), 1, km);
            if (is_gz) { const int64_t t = km.auto_cutoff(); km.clean((uint64_t)(t < 0 ? 0 : t)); }
            nk = km.size();
        }
        if (nk == 0) { fprintf(stderr, "%s has no k-mers: skipped\n", kv.first.c_str()); if (ks) cid_kmerset_destroy(ks); continue; }
        for (int hv = 0; hv < CID_HASH_VARIANTS; ++hv) {
            CID_TRY(cid_index_set_hash_variant(b.index, hv));
            if (ks) CID_TRY(cid_search_count_set(ctx, b.index, ks, hits.data(), nullptr, nullptr, nullptr));
            else CID_TRY(cid_search_count(ctx, b.index, km.keys(), nullptr, km.size(), hits.data(), nullptr, nullptr, nullptr));
            const double frac = (double)hits[colour] / (double)nk;
            printf("%s\t%s\t%llu\t%llu\t%.4f\n", variant_names[hv], kv.first.c_str(), (unsigned long long)nk, (unsigned long long)hits[colour], frac);
            if (frac < worst[hv]) worst[hv] = frac;
        }
        if (ks) cid_kmerset_destroy(ks);
        ++n_checked;
    }
    CID_TRY(cid_index_set_hash_variant(b.index, CID_HASH_XXH3_V08));
    return n_checked;
}

Bigsi build_single(cid_ctx *ctx, const std::string &ref_tsv, uint64_t bloom, uint64_t hashes, uint64_t k, uint8_t quality,
                   int64_t cutoff, int hash_variant, uint64_t m_size) {
    const auto refs = tab_to_map(ref_tsv);
    Bigsi b;
    b.bloom_size = bloom; b.num_hash = hashes; b.k_size = k; b.m_size = m_size;
    for (auto &kv : refs) b.colors.push_back(kv.first);
    b.n_ref_kmers.assign(b.colors.size(), 0);
    CID_TRY(cid_index_create(ctx, bloom, (uint32_t)hashes, (uint32_t)k, (uint32_t)b.colors.size(), hash_variant, &b.index));
    if (m_size) CID_TRY(cid_index_set_minimizer(b.index, (uint32_t)m_size));   // the inserts below then key on find_minimizer(kmer, m)
    uint32_t colour = 0, counter = 1;
    // the NEXT accession's input is read (FASTA) or starts inflating (fastq.gz) on a helper thread while the GPU counts and inserts
    // this one's k-mers
    auto gz_of = [](const std::vector<std::string> &v) { return v.size() == 2 || (v[0].size() >= 2 && v[0].compare(v[0].size() - 2, 2, "gz") == 0); };
    std::future<std::vector<std::string>> ahead;
    auto look_ahead = [&](std::map<std::string, std::vector<std::string>>::const_iterator it) {
        if (it == refs.end() || !gpu_counting_enabled(k)) return;
        const std::vector<std::string> &v = it->second;
        if (gz_of(v) && k <= 32 && read_id_mt_pe::device_fastq_wanted(v, v.size())) {   // block gzip: the members go up compressed (count_fastq_gpu)
            for (const std::string &f : v)
                BgzfMemberReader::prefetch(f, read_id_mt_pe::device_fastq_stretch_bytes(0), read_id_mt_pe::device_fastq_host_share(),
                                           read_id_mt_pe::device_fastq_host_threads(v.size()));
        } else if (gz_of(v)) for (const std::string &f : v) LineReader::prefetch(f);
        else { const std::string path = v[0]; ahead = std::async(std::launch::async, [path] { return read_fasta(path); }); }
    };
    look_ahead(refs.begin());
    for (auto it = refs.begin(); it != refs.end(); ++it) {
        const auto &kv = *it;
        fprintf(stderr, "Adding %s to index (%u/%zu)\n", kv.first.c_str(), counter++, refs.size());
        const std::vector<std::string> &v = kv.second;
        const bool is_gz = gz_of(v);
        cid_kmerset *ks = nullptr;
        std::vector<std::string> fasta_now;
        if (gpu_counting_enabled(k) && !is_gz) fasta_now = ahead.get();
        look_ahead(std::next(it));
        if (gpu_counting_enabled(k))
            ks = is_gz ? count_fastq_gpu(ctx, k, v[0], v.size() == 2 ? &v[1] : nullptr, quality) : count_fasta_gpu(ctx, k, fasta_now);
        if (ks) {  // the accession's k-mer map never leaves HBM: count, clean, Bloom-insert
            if (is_gz) {
                uint64_t t = (uint64_t)(cutoff < 0 ? 0 : cutoff);
                if (cutoff == -1) { const int64_t a = auto_cutoff_gpu(ks); if (a < 0) die("auto_cutoff: histogram too short"); t = (uint64_t)a; }
                CID_TRY(cid_kmerset_clean(ks, t));
            } else if (cutoff != -1) {
                CID_TRY(cid_kmerset_clean(ks, (uint64_t)cutoff));   // build.rs:86-91: FASTA is only cleaned with an explicit -f
            }
            uint64_t nk = 0;
            CID_TRY(cid_kmerset_size(ks, &nk));
            b.n_ref_kmers[colour] = (m_size && is_gz) ? 0 : nk;   // build_single_mini records it for FASTA accessions only (Q13)
            CID_TRY(cid_index_insert_kmerset(b.index, ks, colour));
            cid_kmerset_destroy(ks);
        } else {
            KmerMap km((uint32_t)k);
            auto clean_reads = [&]() {
                if (cutoff == -1) { const int64_t t = km.auto_cutoff(); if (t < 0) die("auto_cutoff: histogram too short"); km.clean((uint64_t)t); }
                else km.clean((uint64_t)cutoff);
            };
            if (v.size() == 2) { kmers_fq_pe_qual(v[0], v[1], quality, km); clean_reads(); }
            else if (is_gz) { kmers_from_fq_qual(v[0], quality, km); clean_reads(); }
            else {
                kmerize_vector(read_fasta(v[0]), 1, km);
                if (cutoff != -1) km.clean((uint64_t)cutoff);
            }
            b.n_ref_kmers[colour] = (m_size && is_gz) ? 0 : km.size();
            CID_TRY(cid_index_insert_kmers(b.index, km.keys(), colour, km.size()));
        }
        ++colour;
    }
    LineReader::drop_prefetched();
    BgzfMemberReader::drop_prefetched();
    return b;
}

}  // namespace colorid
