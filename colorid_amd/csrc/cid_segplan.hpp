// The segmented searches' offsets on the host: the one check of seg_off and of group_off, and the one walk that cuts a slice of segments
// into upload chunks with offsets of their own.  Segment s is the k-mers [seg_off[s], seg_off[s + 1]), group g the segments [group_off[g],
// group_off[g + 1]).  And the one lookup the kernels share with it: the segment of a k-mer (segment_of, host and device: cid_segwalk.hpp).
// Plain integer C++ (no HIP types), as cid_readbatch.hpp: also compiled with g++ by tests/test_segplan_cpu.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cid_records.hpp"   // CID_HD

namespace cid {

// which rule an offset array broke, and where: `at` is the segment or the group — for OFF_WRONG_END the value the array ends at
enum OffRule { OFF_OK = 0, OFF_FIRST_NONZERO = 1, OFF_DECREASES = 2, OFF_TOO_LONG = 3, OFF_WRONG_END = 4 };
struct OffFault { OffRule rule = OFF_OK; uint64_t at = 0; };

// seg_off[0] == 0 first; then per segment, in this order: it does not decrease; it has fewer than max_len entries.  Reads seg_off[0 .. n_segs]
inline OffFault check_seg_off(const uint64_t *seg_off, size_t n_segs, uint64_t max_len) {
    if (seg_off[0] != 0) return OffFault{OFF_FIRST_NONZERO, 0};
    for (size_t s = 0; s < n_segs; ++s) {
        if (seg_off[s + 1] < seg_off[s]) return OffFault{OFF_DECREASES, s};
        if (seg_off[s + 1] - seg_off[s] >= max_len) return OffFault{OFF_TOO_LONG, s};
    }
    return OffFault{};
}
// The segment that holds `kmer`: the last s in [0, n_segs) with seg_off[s] <= kmer, so that ties — empty segments — resolve to the last
// equal offset.  n_segs >= 1.  The result is in [0, n_segs) whatever seg_off holds (the kernels rely on that, not on the host's check:
// the device-pointer forms never see the offsets on the host); reads seg_off[1 .. n_segs - 1] at most.
CID_HD uint64_t segment_of(const uint64_t *seg_off, uint64_t n_segs, uint64_t kmer) {
    uint64_t lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (seg_off[mid] <= kmer) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// group_off[0] == 0 first; then no group decreases; last, the array ends at n_segs.  Reads group_off[0 .. n_groups]
inline OffFault check_group_off(const uint64_t *group_off, size_t n_groups, size_t n_segs) {
    if (group_off[0] != 0) return OffFault{OFF_FIRST_NONZERO, 0};
    for (size_t g = 0; g < n_groups; ++g)
        if (group_off[g + 1] < group_off[g]) return OffFault{OFF_DECREASES, g};
    return group_off[n_groups] == n_segs ? OffFault{} : OffFault{OFF_WRONG_END, group_off[n_groups]};
}

// One upload chunk: the k-mers [k0, k0 + nk) of the whole array, in the segments [seg0, seg0 + n_loc), whose n_loc + 1 offsets start at loc[loc0]
struct SegPiece { size_t k0, nk, seg0, n_loc, loc0; };

// The segments [s0, s1) of a checked seg_off, their k-mers cut into chunks of `chunk` (>= 1) k-mers.  loc: first the slice's true offsets,
// seg_off[s0 .. s1] as they are (the segments' lengths, for a kernel that ends the slice); then per piece the offsets of its segments
// clipped to the piece and counted from its first k-mer, so the parts of a segment that a chunk boundary cuts add up to it.  A piece
// begins and ends with a segment it holds k-mers of; a slice without k-mers has no pieces.
inline void plan_slice(const uint64_t *seg_off, size_t s0, size_t s1, size_t chunk, std::vector<uint64_t> &loc, std::vector<SegPiece> &pieces) {
    loc.assign(seg_off + s0, seg_off + s1 + 1);
    pieces.clear();
    size_t sa = s0;
    for (uint64_t k0 = seg_off[s0]; k0 < seg_off[s1]; k0 += chunk) {
        const uint64_t k1 = std::min<uint64_t>(seg_off[s1], k0 + chunk);
        while (seg_off[sa + 1] <= k0) ++sa;          // the segment that holds k-mer k0 (k0 < seg_off[s1]: sa < s1)
        size_t sb = sa;
        while (seg_off[sb + 1] < k1) ++sb;           // the one that holds k-mer k1 - 1 (k1 <= seg_off[s1]: sb < s1)
        pieces.push_back(SegPiece{(size_t)k0, (size_t)(k1 - k0), sa, sb - sa + 1, loc.size()});
        for (size_t s = sa; s <= sb + 1; ++s) loc.push_back(std::min(std::max(seg_off[s], k0), k1) - k0);
    }
}

}  // namespace cid
