// Host-side integer helpers (no HIP types): the exact-modulo constants, the row-stride rule and the divisor rule of `fold`.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace cid {

struct ModMagicHost {
    uint64_t m, magic;
    uint32_t shift, flags;  // flags: 1 = power of two, 2 = add step (same meaning as cid::ModMagic)
};

// Round-up multiply-shift constants for an exact unsigned 64-bit `x % m` (Granlund–Montgomery):
//   q = mulhi64(x, magic); if (add) q = (((x - q) >> 1) + q) >> shift; else q >>= shift;  r = x - q*m.
inline ModMagicHost make_mod_magic(uint64_t m) {
    ModMagicHost mm{m, 0, 0, 0};
    if ((m & (m - 1)) == 0) { mm.flags = 1; return mm; }  // includes m == 1
    const uint32_t fl = 63u - (uint32_t)__builtin_clzll(m);
    const unsigned __int128 num = (unsigned __int128)1 << (64 + fl);
    uint64_t prop = (uint64_t)(num / m);
    const uint64_t rem = (uint64_t)(num % m);
    const uint64_t e = m - rem;
    mm.shift = fl;
    if (e >= ((uint64_t)1 << fl)) {
        prop += prop;
        const uint64_t twice = rem + rem;
        if (twice >= m || twice < rem) prop += 1;
        mm.flags = 2;
    }
    mm.magic = prop + 1;
    return mm;
}

// u64 words per matrix row: 1 for <= 64 colours, else the next power of two >= ceil(C/64) (2..128 words); beyond
// 8192 colours ("wide" rows) a multiple of 128 words = whole KiB, covered by one wave in rs/128 steps.
inline uint32_t row_stride_words(uint32_t n_colors) {
    const uint32_t w64 = (n_colors + 63u) / 64u;
    if (w64 <= 1) return 1;
    if (w64 > 128) return (w64 + 127u) / 128u * 128u;
    uint32_t rs = 2;
    while (rs < w64) rs <<= 1;
    return rs;
}

// `fold`: the rows of an index of m rows fold onto m2 rows when m2 divides m — (h % m) % m2 == h % m2 for every hash h then, so
// OR-ing row r into row r % m2 gives the matrix `build` makes at m2.  The factor m / m2, or 0 when m2 is 0 or does not divide m.
inline uint64_t fold_factor(uint64_t m, uint64_t m2) { return m && m2 && m % m2 == 0 ? m / m2 : 0; }

// The divisors of m, ascending (m >= 1): trial division up to sqrt(m) — at most 65536 steps for a Bloom size (<= 2^32).
inline std::vector<uint64_t> divisors_of(uint64_t m) {
    std::vector<uint64_t> lo, hi;
    for (uint64_t d = 1; d <= m / d; ++d)
        if (m % d == 0) {
            lo.push_back(d);
            if (d != m / d) hi.push_back(m / d);
        }
    lo.insert(lo.end(), hi.rbegin(), hi.rend());
    return lo;
}

// The divisors of m next to s: the largest one <= s (0: there is none, s == 0) and the smallest one >= s (0: none, s > m).
inline void nearest_divisors(uint64_t m, uint64_t s, uint64_t &below, uint64_t &above) {
    below = above = 0;
    for (const uint64_t d : divisors_of(m)) {
        if (d <= s) below = d;
        if (d >= s && !above) above = d;
    }
}

}  // namespace cid
