// Stand-alone check (g++ -fsanitize=address,undefined) that cid_readbatch.hpp never uses an unchecked read_seq0 entry as an index:
// seq_off and read_seq0 are heap arrays of EXACTLY n_seqs + 1 and n_reads + 1 entries, so a read past either is a sanitizer report.
// Every malformed batch must be refused with the right rule and index; exit status 0 = all as expected.  Test infrastructure only.
#include "../../colorid_amd/csrc/cid_readbatch.hpp"

#include <cstdio>
#include <cstring>
#include <memory>

static int failures = 0;

static void expect(const char *what, size_t where, const cid::BatchFault &f, cid::BatchRule rule, uint64_t at) {
    if (f.rule == rule && f.at == at) return;
    fprintf(stderr, "%s, bad entry at read %zu: rule %d at %llu, expected rule %d at %llu\n", what, where, (int)f.rule, (unsigned long long)f.at, (int)rule,
            (unsigned long long)at);
    ++failures;
}

int main() {
    const size_t n_reads = 9, n_seqs = 2 * n_reads;   // paired reads of 40 + 25 bases
    const uint32_t k = 21;
    for (const size_t bad : {(size_t)0, (size_t)4, n_reads - 1})
        for (int kind = 0; kind < 4; ++kind) {
            std::unique_ptr<uint64_t[]> so(new uint64_t[n_seqs + 1]), r0(new uint64_t[n_reads + 1]), prefix(new uint64_t[n_reads + 1]);
            for (size_t s = 0; s <= n_seqs; ++s) so[s] = (s / 2) * 65 + (s % 2) * 40;
            for (size_t r = 0; r <= n_reads; ++r) r0[r] = 2 * r;
            cid::BatchRule rule = cid::BATCH_OK;
            uint64_t at = 0;
            const char *what = "";
            switch (kind) {
            case 0: what = "read_seq0 decreases"; r0[bad] += 1; r0[bad + 1] = r0[bad] - 1; rule = cid::BATCH_READ0_DECREASES; at = bad; break;
            case 1: what = "read_seq0 past n_seqs"; r0[bad + 1] = n_seqs + 1 + 1000000 * bad; rule = cid::BATCH_READ0_PAST_SEQS; at = bad; break;
            case 2: what = "read_seq0 far past n_seqs"; r0[bad + 1] = ~0ull; rule = cid::BATCH_READ0_PAST_SEQS; at = bad; break;
            case 3: what = "seq_off decreases"; so[2 * bad] += 1; so[2 * bad + 1] = so[2 * bad] - 1; rule = cid::BATCH_SEQ_OFF_DECREASES; at = 2 * bad; break;
            }
            const cid::HostOffsets h{so.get(), n_seqs, r0.get(), n_reads};
            for (const uint32_t stride : {1u, 3u}) {
                expect(what, bad, cid::walk_batch(h, k, stride).fault, rule, at);
                expect(what, bad, cid::walk_batch(h, k, stride, prefix.get()).fault, rule, at);
            }
            std::vector<uint64_t> so_out, r0_out;
            uint64_t base;
            expect(what, bad, cid::rebase_batch(h, 0, n_reads, so_out, r0_out, &base), rule, at);
            expect(what, bad, cid::rebase_batch(h, bad, bad + 1, so_out, r0_out, &base), rule, at);
            // a range that ends before the bad read, and an empty one AT it, are fine and touch nothing behind a bad entry
            expect(what, bad, cid::rebase_batch(h, 0, bad, so_out, r0_out, &base), cid::BATCH_OK, 0);
            expect(what, bad, cid::rebase_batch(h, bad + 1, bad + 1, so_out, r0_out, &base), cid::BATCH_OK, 0);
        }
    // the well-formed batch passes, an empty batch reads nothing at all
    {
        std::unique_ptr<uint64_t[]> so(new uint64_t[n_seqs + 1]), r0(new uint64_t[n_reads + 1]);
        for (size_t s = 0; s <= n_seqs; ++s) so[s] = (s / 2) * 65 + (s % 2) * 40;
        for (size_t r = 0; r <= n_reads; ++r) r0[r] = 2 * r;
        const cid::BatchSizes z = cid::walk_batch(cid::HostOffsets{so.get(), n_seqs, r0.get(), n_reads}, k, 1);
        if (z.fault.rule || z.max_bases != 65 || z.max_win != 20 + 5 || z.total_win != n_reads * 25) { fprintf(stderr, "well-formed batch: wrong sizes\n"); ++failures; }
        expect("empty batch", 0, cid::walk_batch(cid::HostOffsets{nullptr, 0, nullptr, 0}, k, 1).fault, cid::BATCH_OK, 0);
    }
    if (failures) return 1;
    puts("readbatch: every malformed batch refused before it was dereferenced");
    return 0;
}
