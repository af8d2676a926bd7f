// Stand-alone check (g++ -fsanitize=address,undefined) that cid_segplan.hpp reads nothing beyond the n_segs + 1 entries of seg_off and
// the n_groups + 1 of group_off: both are heap arrays of EXACTLY that many entries, so a read past either is a sanitizer report.  Every
// malformed array must be refused with the right rule and index, plan_slice must tile every slice of a handful of layouts, and the
// kernels' lookup (segment_of) must stay inside the n_segs entries it may read and inside [0, n_segs) with what it returns; exit
// status 0 = all as expected.  Test infrastructure only.
#include "../../colorid_amd/csrc/cid_segplan.hpp"

#include <cstdio>
#include <memory>

static int failures = 0;

static void expect(const char *what, size_t where, const cid::OffFault &f, cid::OffRule rule, uint64_t at) {
    if (f.rule == rule && f.at == at) return;
    fprintf(stderr, "%s, bad entry at %zu: rule %d at %llu, expected rule %d at %llu\n", what, where, (int)f.rule, (unsigned long long)f.at, (int)rule,
            (unsigned long long)at);
    ++failures;
}

static std::unique_ptr<uint64_t[]> exact(const std::vector<uint64_t> &v) {
    std::unique_ptr<uint64_t[]> a(new uint64_t[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) a[i] = v[i];
    return a;
}

// every slice of per_slice segments, cut into chunks: the pieces tile the slice's k-mers and each piece's offsets run from 0 to nk
static void walk(const char *what, const std::vector<uint64_t> &lens, size_t per_slice, size_t chunk) {
    std::vector<uint64_t> off(1, 0);
    for (const uint64_t n : lens) off.push_back(off.back() + n);
    const size_t n_segs = lens.size();
    const std::unique_ptr<uint64_t[]> so = exact(off);
    expect(what, 0, cid::check_seg_off(so.get(), n_segs, 1ull << 32), cid::OFF_OK, 0);
    std::vector<uint64_t> loc;
    std::vector<cid::SegPiece> pieces;
    for (size_t s0 = 0; s0 < n_segs; s0 += per_slice) {
        const size_t s1 = std::min(n_segs, s0 + per_slice);
        cid::plan_slice(so.get(), s0, s1, chunk, loc, pieces);
        bool ok = loc.size() >= s1 - s0 + 1;
        for (size_t s = s0; ok && s <= s1; ++s) ok = loc[s - s0] == off[s];
        uint64_t next = off[s0];
        size_t used = s1 - s0 + 1;
        for (const cid::SegPiece &p : pieces) {
            ok = ok && p.k0 == next && p.nk >= 1 && p.nk <= chunk && p.loc0 == used && p.seg0 >= s0 && p.seg0 + p.n_loc <= s1 &&
                 p.loc0 + p.n_loc + 1 <= loc.size() && loc[p.loc0] == 0 && loc[p.loc0 + p.n_loc] == p.nk;
            if (!ok) break;
            next += p.nk;
            used += p.n_loc + 1;
        }
        ok = ok && next == off[s1] && used == loc.size();
        if (!ok) { fprintf(stderr, "%s: per_slice %zu, chunk %zu, slice at %zu: the pieces do not tile it\n", what, per_slice, chunk, s0); ++failures; }
    }
}

// segment_of over a heap array of EXACTLY n_segs entries (it never needs seg_off[n_segs]): with true offsets every k-mer lands in the
// segment that holds it; with offsets that break every rule the result still indexes [0, n_segs)
static void lookup(const char *what, const std::vector<uint64_t> &lens) {
    std::vector<uint64_t> off(1, 0), holder;
    for (size_t s = 0; s < lens.size(); ++s) {
        off.push_back(off.back() + lens[s]);
        holder.insert(holder.end(), lens[s], s);
    }
    const size_t n_segs = lens.size();
    off.pop_back();
    const std::unique_ptr<uint64_t[]> so = exact(off);
    for (size_t kmer = 0; kmer < holder.size(); ++kmer)
        if (cid::segment_of(so.get(), n_segs, kmer) != holder[kmer]) { fprintf(stderr, "%s: k-mer %zu is not in segment %zu\n", what, kmer, (size_t)holder[kmer]); ++failures; }
    std::vector<uint64_t> bad(n_segs);
    for (size_t s = 0; s < n_segs; ++s) bad[s] = s % 3 == 0 ? ~0ull : (n_segs - s) * 7;   // decreasing, huge, first entry not 0
    const std::unique_ptr<uint64_t[]> sb = exact(bad);
    for (const uint64_t kmer : {0ull, 1ull, 63ull, 64ull, 1000ull, 1ull << 32, ~0ull})
        if (cid::segment_of(sb.get(), n_segs, kmer) >= n_segs) { fprintf(stderr, "%s: malformed offsets took k-mer %llu out of range\n", what, (unsigned long long)kmer); ++failures; }
}

int main() {
    const size_t n = 9;                                   // nine segments of 40 k-mers; three groups of three
    std::vector<uint64_t> good_seg, good_grp;
    for (size_t s = 0; s <= n; ++s) good_seg.push_back(40 * s);
    for (size_t g = 0; g <= n / 3; ++g) good_grp.push_back(3 * g);
    for (const uint64_t max_len : {1ull << 32, (1ull << 32) - 128})
        for (const size_t bad : {(size_t)0, (size_t)4, n - 1}) {
            std::vector<uint64_t> v = good_seg;
            if (bad) v[bad + 1] = v[bad] - 1;
            else v[0] = 50;                               // segment 0 can decrease only from a non-zero first entry: that rule comes first
            expect("seg_off", bad, cid::check_seg_off(exact(v).get(), n, max_len), bad ? cid::OFF_DECREASES : cid::OFF_FIRST_NONZERO, bad);
            v = good_seg;
            for (size_t s = bad + 1; s <= n; ++s) v[s] += max_len - 40;          // segment `bad` has max_len entries
            expect("seg_off too long", bad, cid::check_seg_off(exact(v).get(), n, max_len), cid::OFF_TOO_LONG, bad);
            for (size_t s = bad + 1; s <= n; ++s) v[s] -= 1;                     // one fewer is fine
            expect("seg_off just short enough", bad, cid::check_seg_off(exact(v).get(), n, max_len), cid::OFF_OK, 0);
            if (bad + 2 <= n) {                                                  // too long at `bad`, decreasing right after it
                v = good_seg;
                v[bad + 1] = v[bad] + max_len;
                expect("seg_off too long, then decreases", bad, cid::check_seg_off(exact(v).get(), n, max_len), cid::OFF_TOO_LONG, bad);
            }
        }
    {
        std::vector<uint64_t> v = good_seg;
        v[1] = 30; v[2] = 20;                                                    // decreases at segment 1
        expect("seg_off decreases", 1, cid::check_seg_off(exact(v).get(), n, 1ull << 32), cid::OFF_DECREASES, 1);
        expect("seg_off, no segments", 0, cid::check_seg_off(exact({0}).get(), 0, 1ull << 32), cid::OFF_OK, 0);
        expect("seg_off, no segments, non-zero", 0, cid::check_seg_off(exact({7}).get(), 0, 1ull << 32), cid::OFF_FIRST_NONZERO, 0);
    }
    const size_t ng = n / 3;
    expect("group_off", 0, cid::check_group_off(exact(good_grp).get(), ng, n), cid::OFF_OK, 0);
    for (const size_t bad : {(size_t)0, (size_t)1, ng - 1}) {
        std::vector<uint64_t> v = good_grp;
        v[bad] += 2; v[bad + 1] = v[bad] - 1;
        expect("group_off decreases", bad, cid::check_group_off(exact(v).get(), ng, n), bad ? cid::OFF_DECREASES : cid::OFF_FIRST_NONZERO, bad ? bad : 0);
    }
    {
        std::vector<uint64_t> v = good_grp;
        v[ng] = n + 1;
        expect("group_off past the segments", ng, cid::check_group_off(exact(v).get(), ng, n), cid::OFF_WRONG_END, n + 1);
        v[ng] = n - 1;
        expect("group_off short of the segments", ng, cid::check_group_off(exact(v).get(), ng, n), cid::OFF_WRONG_END, n - 1);
        v[1] = 7; v[2] = 5;                                                      // decreases AND ends wrong: the order decides
        expect("group_off decreases and ends wrong", 1, cid::check_group_off(exact(v).get(), ng, n), cid::OFF_DECREASES, 1);
        expect("group_off, no groups, no segments", 0, cid::check_group_off(exact({0}).get(), 0, 0), cid::OFF_OK, 0);
    }
    const std::vector<uint64_t> mixed = {0, 0, 1, 63, 64, 0, 0, 0, 65, 128, 200, 1, 0, 64, 64, 0, 0};
    for (const size_t per_slice : {(size_t)1, (size_t)3, (size_t)8, mixed.size()})
        for (const size_t chunk : {(size_t)64, (size_t)128}) {
            walk("mixed lengths", mixed, per_slice, chunk);
            walk("only empty segments", {0, 0, 0, 0, 0}, per_slice, chunk);
            walk("boundary on a boundary", {64, 64, 128, 64}, per_slice, chunk);
            walk("one segment over three chunks", {3, 3 * chunk - 10, 5}, per_slice, chunk);
        }
    lookup("mixed lengths", mixed);
    lookup("one segment", {5});
    lookup("a trailing empty segment", {1, 0});
    lookup("leading empty segments", {0, 0, 64, 64, 0, 128, 1});
    if (failures) return 1;
    puts("segplan: every malformed array refused within its bounds, every slice tiled, every k-mer in its segment");
    return 0;
}
