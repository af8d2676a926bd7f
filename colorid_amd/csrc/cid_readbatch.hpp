// A read batch's offsets on the host (no HIP types): the one walk that validates them and sizes the batch, and the one rebase of a
// range of reads to offsets of its own.  Read r is the sequences [read_seq0[r], read_seq0[r + 1]), sequence s the bases
// [seq_off[s], seq_off[s + 1]).  Both functions check an entry of read_seq0 before seq_off is read through it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cid {

struct HostOffsets {
    const uint64_t *seq_off = nullptr;
    uint64_t n_seqs = 0;                  // seq_off has n_seqs + 1 entries; ~0: the caller vouches for its length
    const uint64_t *read_seq0 = nullptr;  // n_reads + 1 entries
    size_t n_reads = 0;
};
// which rule a batch broke, and where: `at` is a read (the two rules of read_seq0) or a sequence (seq_off)
enum BatchRule { BATCH_OK = 0, BATCH_READ0_DECREASES = 1, BATCH_READ0_PAST_SEQS = 2, BATCH_SEQ_OFF_DECREASES = 3 };
struct BatchFault { BatchRule rule = BATCH_OK; uint64_t at = 0; };
struct BatchSizes {
    uint64_t max_bases = 0, max_win = 0, total_win = 0;   // the longest read in bases and in k-mer windows; the windows of the whole batch
    BatchFault fault;                                     // rule != BATCH_OK: refused, the sizes mean nothing
};

// Per read, in this order: read_seq0[r + 1] >= read_seq0[r]; read_seq0[r + 1] <= n_seqs; only then seq_off[s + 1] >= seq_off[s] for
// the read's sequences.  A sequence of len >= k bases has (len - k) / stride_d + 1 windows.  win_prefix (or NULL): n_reads + 1 words,
// [r] = the windows of the reads before r.
// (The walk runs on the caller's thread before anything is launched: a million reads of 150 bases took 2.1 ms in it — beside 5.2 ms of
// kernel — while every sequence paid a 64-bit division by a stride that is 1 unless -d says otherwise: stride 1 does not divide.)
inline BatchSizes walk_batch(const HostOffsets &b, uint32_t k, uint32_t stride_d, uint64_t *win_prefix = nullptr) {
    BatchSizes z;
    const bool every = stride_d == 1;   // no division then
    if (win_prefix) win_prefix[0] = 0;
    for (size_t r = 0; r < b.n_reads; ++r) {
        const uint64_t s0 = b.read_seq0[r], s1 = b.read_seq0[r + 1];
        if (s1 < s0) { z.fault = BatchFault{BATCH_READ0_DECREASES, r}; return z; }
        if (s1 > b.n_seqs) { z.fault = BatchFault{BATCH_READ0_PAST_SEQS, r}; return z; }
        uint64_t win = 0;
        for (uint64_t s = s0; s < s1; ++s) {
            if (b.seq_off[s + 1] < b.seq_off[s]) { z.fault = BatchFault{BATCH_SEQ_OFF_DECREASES, s}; return z; }
            const uint64_t len = b.seq_off[s + 1] - b.seq_off[s];
            if (len >= k) win += every ? len - k + 1 : (len - k) / stride_d + 1;
        }
        const uint64_t bases = s1 > s0 ? b.seq_off[s1] - b.seq_off[s0] : 0;
        if (bases > z.max_bases) z.max_bases = bases;
        if (win > z.max_win) z.max_win = win;
        z.total_win += win;
        if (win_prefix) win_prefix[r + 1] = z.total_win;
    }
    return z;
}

// Reads [lo, hi) of a batch as a batch of their own: seq_off (one entry per sequence + 1) and read_seq0 (hi - lo + 1) starting at 0,
// *base = where the range's bases begin in the batch's.  Validates as it goes, by the rules and in the order of walk_batch.
inline BatchFault rebase_batch(const HostOffsets &b, size_t lo, size_t hi, std::vector<uint64_t> &seq_off, std::vector<uint64_t> &read_seq0,
                               uint64_t *base) {
    seq_off.assign(1, 0);
    read_seq0.assign(hi - lo + 1, 0);
    *base = 0;
    if (hi == lo) return BatchFault{};
    for (size_t r = lo; r < hi; ++r) {
        if (b.read_seq0[r + 1] < b.read_seq0[r]) return BatchFault{BATCH_READ0_DECREASES, r};
        if (b.read_seq0[r + 1] > b.n_seqs) return BatchFault{BATCH_READ0_PAST_SEQS, r};
        read_seq0[r + 1 - lo] = b.read_seq0[r + 1] - b.read_seq0[lo];
    }
    const uint64_t s0 = b.read_seq0[lo], s1 = b.read_seq0[hi];
    seq_off.resize(s1 - s0 + 1);
    for (uint64_t s = s0; s < s1; ++s) {
        if (b.seq_off[s + 1] < b.seq_off[s]) return BatchFault{BATCH_SEQ_OFF_DECREASES, s};
        seq_off[s + 1 - s0] = b.seq_off[s + 1] - b.seq_off[s0];
    }
    *base = b.seq_off[s0];
    return BatchFault{};
}

}  // namespace cid
