// The .bxi / .mxi row record, defined once for the kernels that read or write it (cid_index.hip, cid_pairs.hip, cid_reports.hip), the API
// layer that stages it (cid_api_common.hpp: stage_records) and the host's file reader (host/bigsi_io.cpp): its layout, its check, the tail
// mask of a row's last word, and the walk over the runs of a 32-bit mask behind `merge`'s deposit and `subset`'s extract.  Plain integer
// C++ (no HIP types): also compiled with g++ by the CPU unit test of this arithmetic (tests/cpu_shim/).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CID_HD __host__ __device__ __forceinline__
#else
#define CID_HD inline
#endif

namespace cid {

// record = { u64 row ; u64 n_words ; n_words x u32 ; u64 n_bits } (bincode of (usize, BitVec)), every field 4-byte
// aligned: as u32 words, the row at 0, the word count at 2, the payload at kRecordPayload, the bit count behind it.
constexpr uint32_t kRecordPayload = 4;
CID_HD uint64_t record_words(uint32_t w32) { return 6ull + w32; }                                            // the stride, in u32 words
CID_HD size_t record_bytes(uint64_t n_colors) { return (size_t)(24u + 4u * ((n_colors + 31u) / 32u)); }   // = 4 * record_words(W32)
CID_HD uint64_t record_row(const uint32_t *rec) { return (uint64_t)rec[0] | ((uint64_t)rec[1] << 32); }

// the n lowest bits, n in 0..32
CID_HD uint32_t low_bits(uint32_t n) { return n == 32u ? 0xFFFFFFFFu : (1u << n) - 1u; }
// the bits of a row's last u32 word that are colours
CID_HD uint32_t tail_mask(uint32_t n_colors) { return low_bits(n_colors % 32u ? n_colors % 32u : 32u); }

// One record — row = record_row(rec), which every caller has read already — against the FILE's shape (w32_rec words, n_colors bits,
// tail = tail_mask(n_colors)) and the index's rows: 1 bad word count | 2 bad bit count | 4 row >= bloom_size | 8 bits past n_colors;
// 0 = well-formed.
CID_HD uint32_t check_record(const uint32_t *rec, uint64_t row, uint32_t w32_rec, uint32_t n_colors, uint64_t bloom_size, uint32_t tail) {
    const uint64_t nw = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
    const uint64_t nbits = (uint64_t)rec[kRecordPayload + w32_rec] | ((uint64_t)rec[kRecordPayload + w32_rec + 1] << 32);
    return (nw != w32_rec ? 1u : 0u) | (nbits != n_colors ? 2u : 0u) | (row >= bloom_size ? 4u : 0u) |
           ((rec[kRecordPayload + w32_rec - 1] & ~tail) ? 8u : 0u);
}

// f(at, len) for every run of set bits [at, at + len) of m, lowest first
template <class F>
CID_HD void for_each_run(uint32_t m, F f) {
    while (m) {
        const uint32_t at = (uint32_t)__builtin_ctz(m);
        const uint32_t rest = m >> at;
        const uint32_t len = rest == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_ctz(~rest);
        f(at, len);
        m &= ~(low_bits(len) << at);
    }
}
// the low popcount(mask) bits of `bits`, spread over the set bits of mask in order (a software pdep)
CID_HD uint32_t deposit_bits(uint32_t bits, uint32_t mask) {
    uint32_t out = 0;
    for_each_run(mask, [&](uint32_t at, uint32_t len) {
        out |= (bits & low_bits(len)) << at;
        bits = len == 32u ? 0u : bits >> len;
    });
    return out;
}
// the bits of `word` under the set bits of mask, packed into the low n = popcount(mask) bits (a software pext); the walk counts n
CID_HD uint32_t extract_bits(uint32_t word, uint32_t mask, uint32_t &n) {
    uint32_t bits = 0;
    n = 0;
    for_each_run(mask, [&](uint32_t at, uint32_t len) {
        bits |= ((word >> at) & low_bits(len)) << n;   // (n < 32 while a run is left)
        n += len;
    });
    return bits;
}

}  // namespace cid
