// CPU unit-test harness (g++) for the segmented searches' offset checks and slice walk: includes the SAME
// colorid_amd/csrc/cid_segplan.hpp the library compiles.  Test infrastructure only; never linked into the product.
#include "../../colorid_amd/csrc/cid_segplan.hpp"

extern "C" {

// out[2] = rule, at
void shim_check_seg_off(const uint64_t *seg_off, uint64_t n_segs, uint64_t max_len, uint64_t *out) {
    const cid::OffFault f = cid::check_seg_off(seg_off, (size_t)n_segs, max_len);
    out[0] = f.rule; out[1] = f.at;
}
void shim_check_group_off(const uint64_t *group_off, uint64_t n_groups, uint64_t n_segs, uint64_t *out) {
    const cid::OffFault f = cid::check_group_off(group_off, (size_t)n_groups, (size_t)n_segs);
    out[0] = f.rule; out[1] = f.at;
}
// out[i] = the segment of kmers[i]
void shim_segment_of(const uint64_t *seg_off, uint64_t n_segs, const uint64_t *kmers, uint64_t n, uint64_t *out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = cid::segment_of(seg_off, n_segs, kmers[i]);
}
// loc_out: room for loc_cap words, pieces_out: 5 words (k0, nk, seg0, n_loc, loc0) for each of piece_cap pieces; out[2] = the
// numbers of loc words and of pieces (nothing is copied when either exceeds its room)
void shim_plan_slice(const uint64_t *seg_off, uint64_t s0, uint64_t s1, uint64_t chunk, uint64_t *loc_out, uint64_t loc_cap, uint64_t *pieces_out,
                     uint64_t piece_cap, uint64_t *out) {
    std::vector<uint64_t> loc(3, 77);                       // stale content: plan_slice starts both afresh
    std::vector<cid::SegPiece> pieces(2, cid::SegPiece{9, 9, 9, 9, 9});
    cid::plan_slice(seg_off, (size_t)s0, (size_t)s1, (size_t)chunk, loc, pieces);
    out[0] = loc.size(); out[1] = pieces.size();
    if (loc.size() > loc_cap || pieces.size() > piece_cap) return;
    for (size_t i = 0; i < loc.size(); ++i) loc_out[i] = loc[i];
    for (size_t i = 0; i < pieces.size(); ++i) {
        const cid::SegPiece &p = pieces[i];
        const uint64_t w[5] = {p.k0, p.nk, p.seg0, p.n_loc, p.loc0};
        for (int j = 0; j < 5; ++j) pieces_out[5 * i + j] = w[j];
    }
}

}  // extern "C"
