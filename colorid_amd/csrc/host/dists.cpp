// Pairwise allele distances and single-linkage clusters of a cgMLST table (`colorid dists -t TABLE -o PREFIX`, `search -s -m --alleles
// PREFIX --dists`): the step after the accessions x loci table.  No reference counterpart (workflows/MLST/process_MLST.py stops at the table).
//   table        PREFIX.raw.tsv / PREFIX.clean.tsv as alleles.cpp writes them: header = an empty first cell, then the loci; per accession its
//                name and one cell per locus; NA or an empty cell = no call
//   codes        per locus the allele texts numbered from 1 in order of first appearance, 0 = no call (AlleleCodes): what cid_dists_* takes
//   compared     for two accessions, the loci at which both have a call;  differ: those of them at which the calls are not the same text
//   PREFIX.dists.tsv, PREFIX.compared.tsv   header = an empty first cell, then the accessions; per accession its name and one integer per
//                accession (differ / compared), written row block by row block: the host never holds an A x A matrix
//   PREFIX.clusters.tsv (--cluster T [--min-compared M])   i and j are linked when compared >= M (at least 1: a pair without a common locus
//                never links) and differ <= T; clusters = connected components, numbered from 1 in order of their first member
//   PREFIX.mst.tsv, PREFIX.mst.nwk (--mst [--min-compared M])   the minimum spanning forest of the graph whose edges are the pairs with
//                compared >= M, under the key (differ, more compared first, earlier accessions first): cid_dists_forest, Borůvka rounds on
//                the device, 8 bytes an accession a round over the bus.  Its edges with differ <= T span exactly the clusters at T.
//   PREFIX.within.tsv (--within T [--min-compared M])   a, b, differ, compared for every unordered pair with compared >= M and differ <= T,
//                a before b in the table, in order of (a's row, b's row): cid_dists_within(CID_DISTS_UPPER) block of rows by block of rows —
//                only those pairs leave the device.  Their components are the clusters at T; the forest's edges of at most T are among them.
//   PREFIX.query.tsv (--query TABLE2 --within T [--min-compared M], `colorid dists` only, nothing else is written)   TABLE2's accessions
//                on TABLE's loci, matched by name, through the same encoder (AlleleCodes::from_files); the device holds the one table of
//                both and cid_dists_within answers for the query's rows: per query accession its neighbours among all the others,
//                nearest first (differ, more compared first, table before query, file order), or one line of dashes
//   PREFIX.closest.tsv (--closest K [--within T] [--min-compared M], K = 1 .. 64)   accession, neighbour, differ, compared: the accessions in
//                table order and under each its up to K nearest among the others with compared >= M (and differ <= T), nearest first in
//                the order of PREFIX.query.tsv; an accession without one gets a line of dashes: cid_dists_closest, K x 16 bytes an
//                accession over the bus.  With --query it cuts every query accession's list in PREFIX.query.tsv to its first K lines,
//                and --within is then optional: without it the K nearest however far they are
//   PREFIX.hist.tsv (--hist [--min-compared M])   loci, differ_pairs, differ_cumulative, compared_pairs: one line for every n = 0 .. L, the
//                empty ones too: the unordered pairs with compared >= M and differ = n, the running sum of that column (= the lines
//                --within n would write), and the unordered pairs of all accessions with compared = n (whatever M is; n = 0: no common
//                locus): cid_dists_hist(CID_DISTS_UPPER) over all rows, 16 bytes a line over the bus.  A table without accessions or
//                loci gets L + 1 lines of zeros
//   PREFIX.levels.tsv (--levels T1,T2,.. [--min-compared M], 1 .. 32 thresholds)   accession, one column T<t> per threshold from the
//                largest t to the smallest, address: in table order, every accession's cluster at each threshold — the `cluster` column
//                of PREFIX.clusters.tsv from --cluster t: single linkage, numbered from 1 in order of the first member — and the
//                numbers joined by '.'.  The levels nest.  From the edges of ONE cid_dists_forest call (the one --mst writes), a
//                union-find over them in key order, read off at each threshold: no row leaves the device
//   --no-matrices   the two A x A files are not made; rows are then fetched for --cluster only
#include "colorid_host.hpp"

#include <algorithm>
#include <cctype>
#include <cstring>
#include <numeric>

namespace colorid {

namespace {

// The one encoder of both entrances: allele text -> code, per locus, in order of first appearance; "" and NA are no call.
class AlleleEncoder {
  public:
    explicit AlleleEncoder(size_t n_loci) : maps_(n_loci) {}
    uint32_t code(size_t locus, const char *text, size_t len) {
        if (len == 0 || (len == 2 && text[0] == 'N' && text[1] == 'A')) return 0;
        auto &m = maps_[locus];
        key_.assign(text, len);   // (looked up first: an emplace makes its node before it looks)
        const auto it = m.find(key_);
        if (it != m.end()) return it->second;
        if (m.size() >= 0xFFFFFFFDull) die("dists: more than 0xFFFFFFFD alleles at one locus");
        return m.emplace(key_, (uint32_t)m.size() + 1u).first->second;
    }
  private:
    std::vector<std::unordered_map<std::string, uint32_t>> maps_;
    std::string key_;
};

void check_shape(size_t n_acc, size_t n_loci) {
    if (n_acc > 0xFFFFFFFFull || n_loci > 0xFFFFFFFFull) die("dists: %zu accessions x %zu loci: more than 2^32 - 1 of either", n_acc, n_loci);
}

FILE *dists_out(const std::string &path) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die("dists: could not create %s", path.c_str());
    setvbuf(f, nullptr, _IOFBF, 1u << 20);
    return f;
}
void dists_close(FILE *f, const std::string &path) {
    if (fclose(f) != 0) die("dists: writing %s failed", path.c_str());
}

// name TAB v[0] TAB v[1] ... NL appended to `line`
void append_row(std::string &line, const std::string &name, const uint32_t *v, size_t n) {
    line += name;
    char buf[12];
    for (size_t j = 0; j < n; ++j) {
        char *p = buf + sizeof buf;
        uint32_t x = v[j];
        do { *--p = (char)('0' + x % 10u); x /= 10u; } while (x);
        *--p = '\t';
        line.append(p, (size_t)(buf + sizeof buf - p));
    }
    line += '\n';
}

// A Newick label: bare, unless it is empty or holds whitespace or one of ( ) [ ] ' : ; , — then in single quotes, every ' doubled.
void append_nwk_name(std::string &out, const std::string &name) {
    bool quote = name.empty();
    for (const char ch : name) quote |= isspace((unsigned char)ch) || strchr("()[]':;,", ch) != nullptr;
    if (!quote) { out += name; return; }
    out += '\'';
    for (const char ch : name) { out += ch; if (ch == '\'') out += '\''; }
    out += '\'';
}

// PREFIX.mst.tsv: the forest's edges (a < b, in edge-key order) by name.  PREFIX.mst.nwk: one line per tree in order of its first
// accession, which is the root; a node is (child,child,..)name:differ with its children in table order, a leaf name:differ, the root
// carries no length.  Written from an explicit stack: a chain of any length does not recurse.
void write_forest(const std::vector<std::string> &names, const std::vector<cid_dists_edge> &edges, const std::string &prefix) {
    const size_t A = names.size();
    const std::string t_path = prefix + ".mst.tsv", n_path = prefix + ".mst.nwk";
    FILE *ft = dists_out(t_path);
    fputs("a\tb\tdiffer\tcompared\n", ft);
    unsigned long long total = 0;
    for (const cid_dists_edge &e : edges) {
        fprintf(ft, "%s\t%s\t%u\t%u\n", names[e.a].c_str(), names[e.b].c_str(), e.differ, e.compared);
        total += e.differ;
    }
    dists_close(ft, t_path);
    // adjacency lists, one run per accession, sorted by the neighbour
    struct Arc { uint32_t to, differ; };
    std::vector<size_t> first(A + 1, 0);
    for (const cid_dists_edge &e : edges) { ++first[e.a + 1]; ++first[e.b + 1]; }
    for (size_t i = 0; i < A; ++i) first[i + 1] += first[i];
    std::vector<Arc> arcs(2 * edges.size());
    {
        std::vector<size_t> fill(first.begin(), first.end() - 1);
        for (const cid_dists_edge &e : edges) {
            arcs[fill[e.a]++] = Arc{e.b, e.differ};
            arcs[fill[e.b]++] = Arc{e.a, e.differ};
        }
    }
    for (size_t i = 0; i < A; ++i)
        std::sort(arcs.begin() + (ptrdiff_t)first[i], arcs.begin() + (ptrdiff_t)first[i + 1], [](const Arc &x, const Arc &y) { return x.to < y.to; });
    FILE *fn = dists_out(n_path);
    struct Frame { uint32_t node, up, differ; size_t next; bool opened; };   // up: the parent (the node itself at the root); next: the arc to look at
    std::vector<bool> seen(A, false);
    std::vector<Frame> stack;
    std::string line;
    char num[16];
    for (size_t root = 0; root < A; ++root) {
        if (seen[root]) continue;
        line.clear();
        stack.push_back(Frame{(uint32_t)root, (uint32_t)root, 0, first[root], false});
        while (!stack.empty()) {
            Frame &f = stack.back();
            seen[f.node] = true;
            while (f.next < first[f.node + 1] && arcs[f.next].to == f.up && f.up != f.node) ++f.next;   // not back up the tree
            if (f.next < first[f.node + 1]) {
                line += f.opened ? ',' : '(';
                f.opened = true;
                const Arc a = arcs[f.next++];
                const uint32_t node = f.node;
                stack.push_back(Frame{a.to, node, a.differ, first[a.to], false});   // (f is not used past this line)
                continue;
            }
            if (f.opened) line += ')';
            append_nwk_name(line, names[f.node]);
            if (f.up != f.node) {
                snprintf(num, sizeof num, ":%u", f.differ);
                line += num;
            }
            stack.pop_back();
        }
        line += ";\n";
        fwrite(line.data(), 1, line.size(), fn);
    }
    dists_close(fn, n_path);
    fprintf(stderr, "dists: minimum spanning forest: %zu trees, %zu edges, total length %llu, written to %s, %s\n", A - edges.size(), edges.size(),
            total, t_path.c_str(), n_path.c_str());
}

// PREFIX.levels.tsv from the forest's edges (in edge-key order, so by differ ascending): the edges of at most t span the clusters at t, so
// one union-find takes the edges in that order and is read off at every threshold on the way, finest first.  The smaller root stays the
// root: a cluster's root is its first member, and numbering the roots as the accessions come by is numbering the clusters from 1 in
// order of their first member.  levels: descending.  Host memory: 4 bytes an accession and level.
void write_levels(const std::vector<std::string> &names, const std::vector<cid_dists_edge> &edges, const std::vector<uint64_t> &levels,
                  uint64_t min_compared, const std::string &prefix) {
    const size_t A = names.size(), n_levels = levels.size();
    std::vector<uint32_t> parent(A), number(A), of(A * n_levels);   // of[i * n_levels + k]: accession i's cluster at levels[k]
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    std::vector<uint32_t> n_clusters(n_levels, 0);
    size_t e = 0;
    for (size_t k = n_levels; k-- > 0;) {
        for (; e < edges.size() && edges[e].differ <= levels[k]; ++e) {
            const uint32_t a = find(edges[e].a), b = find(edges[e].b);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
        std::fill(number.begin(), number.end(), 0u);
        for (size_t i = 0; i < A; ++i) {
            const uint32_t root = find((uint32_t)i);
            if (!number[root]) number[root] = ++n_clusters[k];
            of[i * n_levels + k] = number[root];
        }
    }
    const std::string l_path = prefix + ".levels.tsv";
    FILE *fl = dists_out(l_path);
    std::string line = "accession", said;
    for (size_t k = 0; k < n_levels; ++k) {
        line += "\tT" + std::to_string(levels[k]);
        said += (k ? ", " : "") + std::to_string(n_clusters[k]) + " at <= " + std::to_string(levels[k]);
    }
    line += "\taddress\n";
    fputs(line.c_str(), fl);
    for (size_t i = 0; i < A; ++i) {
        line = names[i];
        std::string address;
        for (size_t k = 0; k < n_levels; ++k) {
            const std::string n = std::to_string(of[i * n_levels + k]);
            line += '\t' + n;
            address += (k ? "." : "") + n;
        }
        line += '\t' + address + '\n';
        fwrite(line.data(), 1, line.size(), fl);
    }
    dists_close(fl, l_path);
    fprintf(stderr, "dists: cluster addresses of %zu accessions (at least %llu shared): %s differing loci, written to %s\n", A,
            (unsigned long long)min_compared, said.c_str(), l_path.c_str());
}

}  // namespace

AlleleCodes AlleleTable::codes(long long max_missing) const {
    AlleleCodes t;
    t.loci.assign(loci_.begin(), loci_.end());
    check_shape(accessions_.size(), t.loci.size());
    AlleleEncoder enc(t.loci.size());
    std::vector<uint32_t> row(t.loci.size());
    for (size_t a = 0; a < accessions_.size(); ++a) {
        const auto &cells = cells_[a];
        size_t na = 0, l = 0;
        auto it = cells.begin();   // ordered as the loci are: a merge walk, as write() does
        for (const std::string &locus : t.loci) {
            row[l] = 0;
            if (it != cells.end() && it->first == locus) {
                if (it->second.n == 1) row[l] = enc.code(l, it->second.allele.data(), it->second.allele.size());
                else ++na;
                ++it;
            } else ++na;
            ++l;
        }
        if (max_missing >= 0 && (long long)na > max_missing) continue;   // not in PREFIX.clean.tsv
        t.accessions.push_back(accessions_[a]);
        t.codes.insert(t.codes.end(), row.begin(), row.end());
    }
    return t;
}

namespace {

// One table file into t, through enc.  on_header gets the file's loci and says, per column of the file, which locus of t it is (kNoLocus:
// the column is not kept); it sets t.loci and makes the encoder where the file is the first.  An accession's loci without a column are no call.
constexpr size_t kNoLocus = ~(size_t)0;
template <typename OnHeader>
void read_table(const std::string &path, AlleleCodes &t, std::unique_ptr<AlleleEncoder> &enc, OnHeader on_header) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("dists: could not open %s", path.c_str());
    char *line = nullptr;
    size_t cap = 0, line_no = 0, n_cols = 0;
    ssize_t n;
    std::unordered_map<std::string, size_t> seen;   // accession -> its line
    std::vector<std::pair<const char *, size_t>> cells;
    std::vector<size_t> to;                         // column of the file -> locus of t
    std::vector<uint32_t> row;
    while ((n = getline(&line, &cap, f)) >= 0) {
        ++line_no;
        size_t len = (size_t)n;
        if (len && line[len - 1] == '\n') --len;
        if (len && line[len - 1] == '\r') --len;
        if (line_no > 1 && len == 0) continue;
        cells.clear();
        for (const char *p = line, *end = line + len;;) {
            const char *tab = static_cast<const char *>(memchr(p, '\t', (size_t)(end - p)));
            cells.emplace_back(p, (size_t)((tab ? tab : end) - p));
            if (!tab) break;
            p = tab + 1;
        }
        if (line_no == 1) {
            if (cells[0].second != 0)
                die("dists: %s has no header: its first line begins with '%.*s', not with an empty cell before the loci", path.c_str(),
                    (int)std::min<size_t>(cells[0].second, 60), cells[0].first);
            std::vector<std::string> loci;
            if (!(cells.size() == 2 && cells[1].second == 0))   // ("\t" alone: a table without loci)
                for (size_t i = 1; i < cells.size(); ++i) loci.emplace_back(cells[i].first, cells[i].second);
            n_cols = loci.size();
            to = on_header(loci);
            continue;
        }
        if (cells.size() != n_cols + 1)
            die("dists: %s line %zu has %zu cells after the name, the header has %zu loci", path.c_str(), line_no, cells.size() - 1, n_cols);
        std::string name(cells[0].first, cells[0].second);
        const auto ins = seen.emplace(name, line_no);
        if (!ins.second)
            die("dists: %s line %zu repeats the accession '%s' of line %zu", path.c_str(), line_no, name.c_str(), ins.first->second);
        t.accessions.push_back(std::move(name));
        row.assign(t.loci.size(), 0u);
        for (size_t l = 0; l < n_cols; ++l)
            if (to[l] != kNoLocus) row[to[l]] = enc->code(to[l], cells[l + 1].first, cells[l + 1].second);
        t.codes.insert(t.codes.end(), row.begin(), row.end());
    }
    free(line);
    fclose(f);
    if (line_no == 0) die("dists: %s has no header: it is empty", path.c_str());
}

// the first table of a run: its header is t's loci
auto first_table(AlleleCodes &t, std::unique_ptr<AlleleEncoder> &enc) {
    return [&t, &enc](const std::vector<std::string> &loci) {
        t.loci = loci;
        enc.reset(new AlleleEncoder(loci.size()));
        std::vector<size_t> to(loci.size());
        std::iota(to.begin(), to.end(), (size_t)0);
        return to;
    };
}

void refuse_repeated_loci(const std::string &path, const std::vector<std::string> &loci) {
    std::unordered_map<std::string, size_t> at;
    for (size_t l = 0; l < loci.size(); ++l) {
        const auto ins = at.emplace(loci[l], l);
        if (!ins.second)
            die("dists: %s repeats the locus '%s' in its header (columns %zu and %zu): with --query the loci are matched by name", path.c_str(),
                loci[l].c_str(), ins.first->second + 1, l + 1);
    }
}

}  // namespace

AlleleCodes AlleleCodes::from_file(const std::string &path) {
    AlleleCodes t;
    std::unique_ptr<AlleleEncoder> enc;
    read_table(path, t, enc, first_table(t, enc));
    check_shape(t.accessions.size(), t.loci.size());
    return t;
}

// `dists --query`: the database table, then the query table's accessions on the database's loci, matched by name, through the one
// encoder (alleles are compared as text per locus).  A query locus the database does not have is ignored; a database locus the query
// lacks is no call for every query accession.
AlleleCodes AlleleCodes::from_files(const std::string &table, const std::string &query, QueryAlign &q) {
    AlleleCodes t;
    std::unique_ptr<AlleleEncoder> enc;
    read_table(table, t, enc, [&](const std::vector<std::string> &loci) {
        refuse_repeated_loci(table, loci);
        return first_table(t, enc)(loci);
    });
    q = QueryAlign{};
    q.table = table;
    q.query = query;
    q.n_table = t.accessions.size();
    read_table(query, t, enc, [&](const std::vector<std::string> &loci) {
        refuse_repeated_loci(query, loci);
        std::unordered_map<std::string, size_t> at;
        for (size_t l = 0; l < t.loci.size(); ++l) at.emplace(t.loci[l], l);
        std::vector<size_t> to(loci.size(), kNoLocus);
        for (size_t l = 0; l < loci.size(); ++l) {
            const auto it = at.find(loci[l]);
            if (it == at.end()) { ++q.only_query; continue; }
            to[l] = it->second;
            ++q.common;
        }
        q.only_table = t.loci.size() - q.common;
        if (q.common == 0)
            die("dists: %s and %s have no locus in common (%zu and %zu loci, matched by name)", table.c_str(), query.c_str(), t.loci.size(), loci.size());
        return to;
    });
    std::unordered_map<std::string, size_t> in_table;
    for (size_t a = 0; a < q.n_table; ++a) in_table.emplace(t.accessions[a], a);
    for (size_t a = q.n_table; a < t.accessions.size(); ++a)
        if (in_table.count(t.accessions[a]))
            die("dists: the accession '%s' is in both %s and %s: a query accession needs a name of its own", t.accessions[a].c_str(), table.c_str(),
                query.c_str());
    check_shape(t.accessions.size(), t.loci.size());
    return t;
}

namespace {

// The pairs of cid_dists_within over the rows [r0, r1), block of rows by block of rows, each block handed to `sink` sorted by (a, b).
// A block is 4096 rows; one that gives more than 2^24 pairs (256 MiB) is asked for again in halves, down to one tile of 64 rows.
template <typename Sink>
uint64_t within_blocks(cid_dists *d, size_t r0, size_t r1, uint64_t threshold, uint64_t min_compared, uint32_t flags, Sink sink) {
    const uint32_t T = (uint32_t)std::min<uint64_t>(threshold, 0xFFFFFFFFull), M = (uint32_t)std::min<uint64_t>(min_compared, 0xFFFFFFFFull);
    std::vector<cid_dists_edge> buf(1u << 16);
    uint64_t total = 0;
    size_t block = 4096;
    for (size_t r = r0; r < r1;) {
        const size_t nr = std::min(block, r1 - r);
        uint64_t n = 0;
        if (cid_dists_within(d, (uint32_t)r, (uint32_t)nr, T, M, flags, buf.data(), buf.size(), &n) != CID_OK) die("cid_dists_within: %s", cid_last_error());
        if (n > buf.size()) {
            if (n > (1ull << 24) && block > 64) { block /= 2; continue; }
            buf.resize((size_t)n);   // come back with room
            continue;
        }
        sink(buf.data(), (size_t)n);
        total += n;
        r += nr;
    }
    return total;
}

constexpr uint32_t kNoNeighbour = 0xFFFFFFFFu;   // cid_dists_edge.b of a rank past an accession's last candidate

// cid_dists_closest over the rows [r0, r1) in blocks of 4096 rows; `sink` gets every row's k entries (the ranks past its candidates
// have b = kNoNeighbour).  Without within the distance is not bounded.
template <typename Sink>
void closest_blocks(cid_dists *d, size_t r0, size_t r1, const DistsOptions &opt, uint64_t min_compared, Sink sink) {
    const uint32_t T = opt.within ? (uint32_t)std::min<uint64_t>(opt.within_threshold, 0xFFFFFFFFull) : 0xFFFFFFFFu;
    const uint32_t M = (uint32_t)std::min<uint64_t>(min_compared, 0xFFFFFFFFull), K = opt.closest;
    const size_t block = 4096;
    std::vector<cid_dists_edge> buf(std::min(block, r1 - r0) * K);
    for (size_t r = r0; r < r1; r += block) {
        const size_t nr = std::min(block, r1 - r);
        if (cid_dists_closest(d, (uint32_t)r, (uint32_t)nr, K, T, M, buf.data()) != CID_OK) die("cid_dists_closest: %s", cid_last_error());
        for (size_t i = 0; i < nr; ++i) sink(r + i, &buf[i * K]);
    }
}

}  // namespace

void dists_run(cid_ctx *ctx, const AlleleCodes &t, const std::string &prefix, const DistsOptions &opt, void (*phase)(const char *)) {
    const size_t A = t.accessions.size(), L = t.loci.size();
    const std::string d_path = prefix + ".dists.tsv", c_path = prefix + ".compared.tsv", k_path = prefix + ".clusters.tsv";
    const bool matrices = !opt.no_matrices;
    FILE *fd = nullptr, *fc = nullptr;
    if (matrices) {
        fd = dists_out(d_path);
        fc = dists_out(c_path);
        std::string header;
        for (const std::string &a : t.accessions) { header += '\t'; header += a; }
        if (A == 0) header += '\t';   // the raw table's convention for a header without columns
        header += '\n';
        fputs(header.c_str(), fd);
        fputs(header.c_str(), fc);
    }
    const uint64_t min_compared = std::max<uint64_t>(opt.min_compared, 1);
    // clustering state, fed row by row: union-find over the links, and per accession its nearest comparable neighbour
    std::vector<uint32_t> parent(opt.cluster ? A : 0);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    constexpr size_t kNone = ~(size_t)0;
    struct Near { size_t j = kNone; uint32_t differ = 0, compared = 0; };
    std::vector<Near> nearest(opt.cluster ? A : 0);
    auto feed = [&](size_t i, const uint32_t *differ, const uint32_t *compared) {
        Near best;
        for (size_t j = 0; j < A; ++j) {
            if (j == i || compared[j] < min_compared) continue;
            if (best.j == kNone || differ[j] < best.differ || (differ[j] == best.differ && compared[j] > best.compared))
                best = Near{j, differ[j], compared[j]};
            if (j > i && differ[j] <= opt.threshold) {
                const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            }
        }
        nearest[i] = best;
    };
    std::string line;
    cid_dists *d = nullptr;
    if (A && L) {
        if (cid_dists_create(ctx, t.codes.data(), (uint32_t)A, (uint32_t)L, &d) != CID_OK) die("cid_dists_create: %s", cid_last_error());
        if (phase) phase("allele codes uploaded");
        // row blocks of whole 64-row tiles, about 32 MiB per matrix; without the matrices only the clusters read rows
        size_t block = std::max<size_t>(64, ((32u << 20) / (A * 4)) & ~(size_t)63);
        block = std::min(block, A);
        if (!matrices && !opt.cluster) block = 0;
        std::vector<uint32_t> differ(block * A), compared(block * A);
        for (size_t r0 = 0; r0 < A && block; r0 += block) {
            const size_t nr = std::min(block, A - r0);
            if (cid_dists_rows(d, (uint32_t)r0, (uint32_t)nr, differ.data(), compared.data()) != CID_OK) die("cid_dists_rows: %s", cid_last_error());
            for (size_t r = 0; r < nr; ++r) {
                if (matrices) {
                    line.clear();
                    append_row(line, t.accessions[r0 + r], &differ[r * A], A);
                    fwrite(line.data(), 1, line.size(), fd);
                    line.clear();
                    append_row(line, t.accessions[r0 + r], &compared[r * A], A);
                    fwrite(line.data(), 1, line.size(), fc);
                }
                if (opt.cluster) feed(r0 + r, &differ[r * A], &compared[r * A]);
            }
        }
    } else if (matrices) {   // no accession or no locus: nothing is compared anywhere, every cell is 0
        const std::vector<uint32_t> zero(A, 0);
        for (size_t i = 0; i < A; ++i) {
            line.clear();
            append_row(line, t.accessions[i], zero.data(), A);
            fwrite(line.data(), 1, line.size(), fd);
            fwrite(line.data(), 1, line.size(), fc);
        }
    }
    if (matrices) {
        dists_close(fd, d_path);
        dists_close(fc, c_path);
        if (phase) phase("distances computed and written");
        fprintf(stderr, "dists: %zu accessions x %zu loci written to %s, %s\n", A, L, d_path.c_str(), c_path.c_str());
    } else {
        if (phase) phase("distances computed");
        fprintf(stderr, "dists: %zu accessions x %zu loci, matrices not written (--no-matrices)\n", A, L);
    }
    if (opt.within) {
        const std::string w_path = prefix + ".within.tsv";
        FILE *fw = dists_out(w_path);
        fputs("a\tb\tdiffer\tcompared\n", fw);
        uint64_t n_pairs = 0;
        if (d)
            n_pairs = within_blocks(d, 0, A, opt.within_threshold, min_compared, CID_DISTS_UPPER, [&](const cid_dists_edge *e, size_t n) {
                for (size_t k = 0; k < n; ++k)
                    fprintf(fw, "%s\t%s\t%u\t%u\n", t.accessions[e[k].a].c_str(), t.accessions[e[k].b].c_str(), e[k].differ, e[k].compared);
            });
        dists_close(fw, w_path);
        if (phase) phase("pairs within the threshold found and written");
        fprintf(stderr, "dists: %llu pairs within %llu differing loci (at least %llu shared), written to %s\n", (unsigned long long)n_pairs,
                (unsigned long long)opt.within_threshold, (unsigned long long)min_compared, w_path.c_str());
    }
    if (opt.closest) {
        const std::string n_path = prefix + ".closest.tsv";
        FILE *fn = dists_out(n_path);
        fputs("accession\tneighbour\tdiffer\tcompared\n", fn);
        uint64_t n_lines = 0;
        size_t without = 0;
        auto none = [&](size_t a) {
            fprintf(fn, "%s\t-\t-\t-\n", t.accessions[a].c_str());
            ++n_lines;
            ++without;
        };
        if (d)
            closest_blocks(d, 0, A, opt, min_compared, [&](size_t a, const cid_dists_edge *e) {
                if (e[0].b == kNoNeighbour) none(a);
                for (uint32_t k = 0; k < opt.closest && e[k].b != kNoNeighbour; ++k, ++n_lines)
                    fprintf(fn, "%s\t%s\t%u\t%u\n", t.accessions[a].c_str(), t.accessions[e[k].b].c_str(), e[k].differ, e[k].compared);
            });
        else
            for (size_t a = 0; a < A; ++a) none(a);   // no locus: nothing is compared
        dists_close(fn, n_path);
        if (phase) phase("closest accessions found and written");
        std::string bound;
        if (opt.within) bound = " within " + std::to_string(opt.within_threshold) + " differing loci";
        fprintf(stderr, "dists: %zu accessions, the %u closest of each%s (at least %llu shared): %llu lines, %zu accessions without a neighbour, written to %s\n",
                A, opt.closest, bound.c_str(), (unsigned long long)min_compared, (unsigned long long)n_lines, without, n_path.c_str());
    }
    if (opt.hist) {
        const std::string h_path = prefix + ".hist.tsv";
        std::vector<uint64_t> differ_hist(L + 1, 0), compared_hist(L + 1, 0);
        if (d && cid_dists_hist(d, 0, (uint32_t)A, (uint32_t)std::min<uint64_t>(min_compared, 0xFFFFFFFFull), CID_DISTS_UPPER, differ_hist.data(),
                                compared_hist.data()) != CID_OK)
            die("cid_dists_hist: %s", cid_last_error());
        FILE *fh = dists_out(h_path);
        fputs("loci\tdiffer_pairs\tdiffer_cumulative\tcompared_pairs\n", fh);
        unsigned long long within = 0, pairs = 0;
        for (size_t n = 0; n <= L; ++n) {
            within += differ_hist[n];
            pairs += compared_hist[n];
            fprintf(fh, "%zu\t%llu\t%llu\t%llu\n", n, (unsigned long long)differ_hist[n], within, (unsigned long long)compared_hist[n]);
        }
        dists_close(fh, h_path);
        if (phase) phase("pairs counted and written");
        fprintf(stderr, "dists: %llu pairs counted, %llu of them left out of the differ columns for sharing fewer than %llu loci, written to %s\n", pairs,
                pairs - within, (unsigned long long)min_compared, h_path.c_str());
    }
    if (opt.cluster) {
        std::vector<uint32_t> size(A, 0), number(A, 0);
        for (size_t i = 0; i < A; ++i) ++size[find((uint32_t)i)];
        size_t n_multi = 0, in_multi = 0;
        uint32_t next = 0;
        FILE *fk = dists_out(k_path);
        fputs("accession\tcluster\tsize\tnearest\tdiffer\tcompared\n", fk);
        for (size_t i = 0; i < A; ++i) {
            const uint32_t root = find((uint32_t)i);
            if (!number[root]) {   // (the root is the component's first member: unions keep the smaller index)
                number[root] = ++next;
                if (size[root] >= 2) { ++n_multi; in_multi += size[root]; }
            }
            const Near &nb = nearest[i];
            if (nb.j == kNone) fprintf(fk, "%s\t%u\t%u\t-\t-\t-\n", t.accessions[i].c_str(), number[root], size[root]);
            else fprintf(fk, "%s\t%u\t%u\t%s\t%u\t%u\n", t.accessions[i].c_str(), number[root], size[root], t.accessions[nb.j].c_str(), nb.differ, nb.compared);
        }
        dists_close(fk, k_path);
        if (phase) phase("clusters written");
        fprintf(stderr, "dists: %zu clusters of 2 or more at <= %llu differing loci hold %zu accessions, written to %s\n", n_multi,
                (unsigned long long)opt.threshold, in_multi, k_path.c_str());
    }
    if (opt.mst || !opt.levels.empty()) {
        // (more than L shared loci are asked of no pair: the forest is then A single accessions, as it is without a locus)
        std::vector<cid_dists_edge> edges(d && min_compared <= L ? A - 1 : 0);
        if (!edges.empty()) {
            uint32_t n_edges = 0, n_rounds = 0;
            if (cid_dists_forest(d, (uint32_t)min_compared, edges.data(), &n_edges, &n_rounds) != CID_OK) die("cid_dists_forest: %s", cid_last_error());
            edges.resize(n_edges);
        }
        if (!opt.levels.empty()) {
            write_levels(t.accessions, edges, opt.levels, min_compared, prefix);
            if (phase) phase("minimum spanning forest computed and cluster addresses written");
        }
        if (opt.mst) {
            write_forest(t.accessions, edges, prefix);
            if (phase) phase(opt.levels.empty() ? "minimum spanning forest computed and written" : "minimum spanning forest written");
        }
    }
    if (d) cid_dists_destroy(d);
}

// `dists --query`: the device holds the one table of D + Q accessions and the query's rows [D, D + Q) are asked for their neighbours
// among all of them (flags = 0: a query accession's pair with another query accession is named from both ends).  Per query accession the
// neighbours are put nearest first: fewer differing loci, then more shared loci, then the lower row — database accessions come before
// query accessions, each in file order — which for a fixed query is the order of the `nearest` column and of the forest's edge key.
// With opt.closest = K the list is cut to its first K: cid_dists_closest over the same rows, which gives them in that order — bounded by
// the threshold only when opt.within is set.
void dists_query_run(cid_ctx *ctx, const AlleleCodes &t, const QueryAlign &q, const std::string &prefix, const DistsOptions &opt,
                     void (*phase)(const char *)) {
    const size_t A = t.accessions.size(), L = t.loci.size(), D = q.n_table, Q = A - D;
    const uint64_t min_compared = std::max<uint64_t>(opt.min_compared, 1);
    const std::string q_path = prefix + ".query.tsv";
    FILE *fq = dists_out(q_path);
    fputs("query\tneighbour\tin\tdiffer\tcompared\n", fq);
    uint64_t n_found = 0;
    size_t next = D, without = 0;   // next: the first query accession without its lines yet
    auto none_up_to = [&](size_t end) {
        for (; next < end; ++next, ++without) fprintf(fq, "%s\t-\t-\t-\t-\n", t.accessions[next].c_str());
    };
    if (Q && L) {
        cid_dists *d = nullptr;
        if (cid_dists_create(ctx, t.codes.data(), (uint32_t)A, (uint32_t)L, &d) != CID_OK) die("cid_dists_create: %s", cid_last_error());
        if (phase) phase("allele codes uploaded");
        std::vector<cid_dists_edge> run;
        if (opt.closest)   // the first K lines of every list: cid_dists_closest's order is the file's
            closest_blocks(d, D, A, opt, min_compared, [&](size_t a, const cid_dists_edge *e) {
                for (uint32_t k = 0; k < opt.closest && e[k].b != kNoNeighbour; ++k, ++n_found)
                    fprintf(fq, "%s\t%s\t%s\t%u\t%u\n", t.accessions[a].c_str(), t.accessions[e[k].b].c_str(), e[k].b < D ? "table" : "query", e[k].differ,
                            e[k].compared);
                if (e[0].b != kNoNeighbour) next = a + 1;
                else none_up_to(a + 1);
            });
        else n_found = within_blocks(d, D, A, opt.within_threshold, min_compared, 0, [&](const cid_dists_edge *e, size_t n) {
            for (size_t k = 0; k < n;) {   // (a block holds whole rows: an accession's neighbours are one run of it)
                size_t end = k;
                while (end < n && e[end].a == e[k].a) ++end;
                none_up_to(e[k].a);
                run.assign(e + k, e + end);
                std::sort(run.begin(), run.end(), [](const cid_dists_edge &x, const cid_dists_edge &y) {
                    if (x.differ != y.differ) return x.differ < y.differ;
                    if (x.compared != y.compared) return x.compared > y.compared;
                    return x.b < y.b;
                });
                for (const cid_dists_edge &x : run)
                    fprintf(fq, "%s\t%s\t%s\t%u\t%u\n", t.accessions[x.a].c_str(), t.accessions[x.b].c_str(), x.b < D ? "table" : "query", x.differ,
                            x.compared);
                next = e[k].a + 1;
                k = end;
            }
        });
        cid_dists_destroy(d);
    }
    none_up_to(A);
    dists_close(fq, q_path);
    if (phase) phase("neighbours of the query accessions found and written");
    if (opt.closest) {
        std::string bound;
        if (opt.within) bound = " within " + std::to_string(opt.within_threshold) + " differing loci";
        fprintf(stderr,
                "dists: %zu query accessions against %zu, %zu loci in common (%zu only in %s, %zu only in %s); %llu neighbours, the %u closest of each%s "
                "(at least %llu shared), %zu queries without one, written to %s\n",
                Q, D, q.common, q.only_table, q.table.c_str(), q.only_query, q.query.c_str(), (unsigned long long)n_found, opt.closest, bound.c_str(),
                (unsigned long long)min_compared, without, q_path.c_str());
        return;
    }
    fprintf(stderr,
            "dists: %zu query accessions against %zu, %zu loci in common (%zu only in %s, %zu only in %s); %llu neighbours within %llu differing loci "
            "(at least %llu shared), %zu queries without one, written to %s\n",
            Q, D, q.common, q.only_table, q.table.c_str(), q.only_query, q.query.c_str(), (unsigned long long)n_found,
            (unsigned long long)opt.within_threshold, (unsigned long long)min_compared, without, q_path.c_str());
}

}  // namespace colorid
