// `collapse`: the plan that takes the colours of a file through an arbitrary many-to-one map into the colours of an index
// (k_put_records_grouped, cid_index.hip), its builder and the evaluation of one output word of one record.  Plain integer C++ (no HIP
// types), as cid_records.hpp: also compiled with g++ by the CPU unit test of the plan (tests/cpu_shim/collapse_main.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "cid_records.hpp"

namespace cid {

// One (file word, group) pair: output bit `bit` of the item's output word is set when the record's payload word s has a bit under mask.
// The items of output u32 word j are items[first, first + n_items) of its GroupWord, in the order of their first file colour; a group
// whose members lie in several file words has several items with the same bit.
struct GroupItem { uint32_t s, mask, bit; };
struct GroupWord { uint32_t first, n_items; };

// 0, or why group_of (n_colors_file entries) is no map onto the n_colors colours of the index
enum GroupPlanFault { kGroupPlanOk = 0, kGroupPlanBeyond = 1, kGroupPlanEmpty = 2 };

// words: one GroupWord per output u32 word; items: at most n_colors_file of them — consecutive file colours of one group in one file
// word fold into one mask.  On a fault `at` is the file colour (beyond) or the index colour (empty) it was found at.
inline GroupPlanFault build_group_plan(const uint32_t *group_of, uint32_t n_colors_file, uint32_t n_colors, std::vector<GroupWord> &words,
                                       std::vector<GroupItem> &items, uint32_t &at) {
    const uint32_t w32_out = (n_colors + 31u) / 32u;
    struct Raw { uint32_t g, s, mask; };
    std::vector<Raw> raw;
    std::vector<uint32_t> last(n_colors, 0xFFFFFFFFu);   // the group's latest item
    for (uint32_t c = 0; c < n_colors_file; ++c) {
        const uint32_t g = group_of[c];
        if (g >= n_colors) { at = c; return kGroupPlanBeyond; }
        if (last[g] == 0xFFFFFFFFu || raw[last[g]].s != c / 32u) {
            last[g] = (uint32_t)raw.size();
            raw.push_back(Raw{g, c / 32u, 0u});
        }
        raw[last[g]].mask |= 1u << (c % 32u);
    }
    for (uint32_t g = 0; g < n_colors; ++g)
        if (last[g] == 0xFFFFFFFFu) { at = g; return kGroupPlanEmpty; }
    words.assign(w32_out, GroupWord{0u, 0u});
    for (const Raw &r : raw) ++words[r.g / 32u].n_items;
    for (uint32_t j = 1; j < w32_out; ++j) words[j].first = words[j - 1].first + words[j - 1].n_items;
    items.resize(raw.size());
    std::vector<uint32_t> fill(w32_out, 0u);
    for (const Raw &r : raw) items[words[r.g / 32u].first + fill[r.g / 32u]++] = GroupItem{r.s, r.mask, r.g % 32u};
    return kGroupPlanOk;
}

// Output word p of one record; word(s) is the record's payload word s
template <class W>
CID_HD uint32_t group_word(const GroupWord p, const GroupItem *items, W word) {
    uint32_t out = 0;
    for (uint32_t t = 0; t < p.n_items; ++t) {
        const GroupItem it = items[p.first + t];   // (it.s < the file's word count: the builder made the items from the file's own colours)
        out |= ((word(it.s) & it.mask) ? 1u : 0u) << it.bit;
    }
    return out;
}

}  // namespace cid
