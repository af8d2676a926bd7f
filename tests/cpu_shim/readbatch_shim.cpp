// CPU unit-test harness (g++) for the walk and the rebase of a read batch's host offsets: includes the SAME
// colorid_amd/csrc/cid_readbatch.hpp the library compiles.  Test infrastructure only; never linked into the product.
#include "../../colorid_amd/csrc/cid_readbatch.hpp"

extern "C" {

// out[6] = max_bases, max_win, total_win, rule, at, 0; prefix: n_reads + 1 words or NULL
void shim_walk(const uint64_t *seq_off, uint64_t n_seqs, const uint64_t *read_seq0, uint64_t n_reads, uint32_t k, uint32_t stride_d, uint64_t *prefix,
               uint64_t *out) {
    const cid::BatchSizes z = cid::walk_batch(cid::HostOffsets{seq_off, n_seqs, read_seq0, (size_t)n_reads}, k, stride_d, prefix);
    out[0] = z.max_bases; out[1] = z.max_win; out[2] = z.total_win; out[3] = z.fault.rule; out[4] = z.fault.at; out[5] = 0;
}
// so_out: room for n_seqs + 1 words, r0_out: hi - lo + 1; out[4] = rule, at, base, the range's number of sequences
void shim_rebase(const uint64_t *seq_off, uint64_t n_seqs, const uint64_t *read_seq0, uint64_t n_reads, uint64_t lo, uint64_t hi, uint64_t *so_out,
                 uint64_t *r0_out, uint64_t *out) {
    std::vector<uint64_t> so, r0;
    uint64_t base = 0;
    const cid::BatchFault f = cid::rebase_batch(cid::HostOffsets{seq_off, n_seqs, read_seq0, (size_t)n_reads}, lo, hi, so, r0, &base);
    out[0] = f.rule; out[1] = f.at; out[2] = base; out[3] = so.size() - 1;
    if (f.rule) return;
    for (size_t i = 0; i < so.size(); ++i) so_out[i] = so[i];
    for (size_t i = 0; i < r0.size(); ++i) r0_out[i] = r0[i];
}

}  // extern "C"
