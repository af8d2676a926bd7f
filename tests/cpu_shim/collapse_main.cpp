// Stand-alone check of `collapse`'s plan (colorid_amd/csrc/cid_collapse.hpp, compiled with g++): plans for chosen many-to-one maps,
// random records evaluated through them as the kernel evaluates them (group_word per output word) and compared with a plain bit-by-bit
// loop; the plan's own invariants; the two refusals.  Exactly-sized heap arrays, so that a sanitizer build sees an index gone astray.
// Exit status 0 when everything agrees; every disagreement is printed.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../colorid_amd/csrc/cid_collapse.hpp"

namespace {

int g_failures = 0;

void fail(const std::string &what, uint32_t ncf, const char *detail) {
    fprintf(stderr, "FAIL %s (n_colors_file %u): %s\n", what.c_str(), ncf, detail);
    ++g_failures;
}

// one map onto nc colours: the plan's invariants, then records through the plan against the plain loop
void check_map(const std::string &what, const std::vector<uint32_t> &group_of, uint32_t nc, std::mt19937_64 &rng) {
    const uint32_t ncf = (uint32_t)group_of.size(), w_in = (ncf + 31u) / 32u, w_out = (nc + 31u) / 32u;
    std::vector<cid::GroupWord> words;
    std::vector<cid::GroupItem> items;
    uint32_t at = 0;
    if (cid::build_group_plan(group_of.data(), ncf, nc, words, items, at) != cid::kGroupPlanOk) return fail(what, ncf, "plan refused");
    if (words.size() != w_out) return fail(what, ncf, "one GroupWord per output word expected");
    if (items.size() > ncf) return fail(what, ncf, "more items than file colours");
    // the items of the words tile the item list; every file colour is under exactly one mask, of its own group's bit and word
    std::vector<uint32_t> seen(ncf, 0u);
    uint32_t next = 0;
    for (uint32_t j = 0; j < w_out; ++j) {
        if (words[j].first != next) return fail(what, ncf, "the words' item runs do not tile the list");
        next += words[j].n_items;
        for (uint32_t t = 0; t < words[j].n_items; ++t) {
            const cid::GroupItem it = items[words[j].first + t];
            if (it.s >= w_in || it.bit >= 32u || it.mask == 0u || 32u * j + it.bit >= nc) return fail(what, ncf, "an item out of range");
            for (uint32_t b = 0; b < 32u; ++b)
                if (it.mask >> b & 1u) {
                    const uint32_t c = 32u * it.s + b;
                    if (c >= ncf || group_of[c] != 32u * j + it.bit) return fail(what, ncf, "a mask bit of another group");
                    ++seen[c];
                }
        }
    }
    if (next != items.size()) return fail(what, ncf, "items beyond the last word's run");
    for (uint32_t c = 0; c < ncf; ++c)
        if (seen[c] != 1u) return fail(what, ncf, "a file colour under no mask or under two");
    // records: random, sparse, all-zero, all-one, one bit
    for (int trial = 0; trial < 40; ++trial) {
        std::vector<uint32_t> rec(w_in);
        for (uint32_t s = 0; s < w_in; ++s) {
            uint32_t v = (uint32_t)rng();
            if (trial % 4 == 1) v &= (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
            if (trial == 2) v = 0u;
            if (trial == 3) v = 0xFFFFFFFFu;
            rec[s] = v;
        }
        if (trial >= 4 && trial < 12) {
            for (uint32_t s = 0; s < w_in; ++s) rec[s] = 0u;
            const uint32_t c = (uint32_t)(rng() % ncf);
            rec[c / 32u] = 1u << (c % 32u);
        }
        rec[w_in - 1] &= cid::tail_mask(ncf);
        std::vector<uint32_t> want(w_out, 0u);
        for (uint32_t c = 0; c < ncf; ++c)
            if (rec[c / 32u] >> (c % 32u) & 1u) want[group_of[c] / 32u] |= 1u << (group_of[c] % 32u);
        for (uint32_t j = 0; j < w_out; ++j) {
            const uint32_t *payload = rec.data();
            const uint32_t got = cid::group_word(words[j], items.data(), [&](uint32_t s) { return payload[s]; });
            if (got != want[j]) return fail(what, ncf, "a record's output word differs from the bit-by-bit loop");
        }
        if (want[w_out - 1] & ~cid::tail_mask(nc)) return fail(what, ncf, "the test's own expectation has bits beyond n_colors");
    }
}

uint32_t groups_of(const std::vector<uint32_t> &m) {
    uint32_t n = 0;
    for (uint32_t g : m) n = g + 1 > n ? g + 1 : n;
    return n;
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    for (const uint32_t ncf : {1u, 31u, 32u, 33u, 64u, 65u, 300u}) {
        std::vector<uint32_t> m(ncf);
        for (uint32_t c = 0; c < ncf; ++c) m[c] = c;
        check_map("identity", m, ncf, rng);
        for (uint32_t c = 0; c < ncf; ++c) m[c] = ncf - 1 - c;
        check_map("reverse permutation", m, ncf, rng);
        for (uint32_t c = 0; c < ncf; ++c) m[c] = 0;
        check_map("all into one", m, 1, rng);
        for (uint32_t c = 0; c < ncf; ++c) m[c] = c / 2;
        check_map("neighbour pairs", m, groups_of(m), rng);
        for (const uint32_t G : {2u, 33u}) {
            if (G > ncf) continue;
            for (uint32_t c = 0; c < ncf; ++c) m[c] = c % G;
            check_map("c mod " + std::to_string(G), m, G, rng);
        }
        if (ncf >= 33) {   // groups across the borders of file words: {31, 32} and, where they exist, {63, 64, 65}; the rest singletons
            std::vector<uint32_t> label(ncf);
            for (uint32_t c = 0; c < ncf; ++c) label[c] = c;
            label[32] = 31;
            if (ncf > 64) label[64] = 63;
            if (ncf > 65) label[65] = 63;
            std::vector<uint32_t> number(ncf, 0xFFFFFFFFu);
            uint32_t n = 0;
            for (uint32_t c = 0; c < ncf; ++c) {
                if (number[label[c]] == 0xFFFFFFFFu) number[label[c]] = n++;
                m[c] = number[label[c]];
            }
            check_map("members at bits 31|32 and 63|64|65", m, n, rng);
        }
        if (ncf >= 4) {   // one group of everything but three singletons: the first, the last and one in the middle; the big group is the LAST colour
            const uint32_t mid = ncf / 2;
            for (uint32_t c = 0; c < ncf; ++c) m[c] = c == 0 ? 0u : c == mid ? 1u : c == ncf - 1 ? 2u : 3u;
            check_map("everything but three singletons", m, 4, rng);
        }
        // refusals: an entry at n_colors, a colour of the index without a member
        {
            std::vector<cid::GroupWord> words;
            std::vector<cid::GroupItem> items;
            uint32_t at = 0xFFFFFFFFu;
            for (uint32_t c = 0; c < ncf; ++c) m[c] = 0;
            m[ncf - 1] = 1;
            if (cid::build_group_plan(m.data(), ncf, 1, words, items, at) != cid::kGroupPlanBeyond || at != ncf - 1)
                fail("refusal", ncf, "an entry == n_colors was not refused at its file colour");
            m[ncf - 1] = 0;
            if (cid::build_group_plan(m.data(), ncf, 2, words, items, at) != cid::kGroupPlanEmpty || at != 1)
                fail("refusal", ncf, "an index colour without a member was not refused");
        }
    }
    if (g_failures) { fprintf(stderr, "%d failure(s)\n", g_failures); return 1; }
    printf("collapse plan: all maps agree\n");
    return 0;
}
