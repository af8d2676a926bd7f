// CPU unit-test harness (g++) for the integer helpers of `colorid fold`: includes the SAME colorid_amd/csrc/cid_host_math.hpp the
// library and the command line compile.  Test infrastructure only; never linked into the product.
#include "../../colorid_amd/csrc/cid_host_math.hpp"

extern "C" {

uint64_t shim_fold_factor(uint64_t m, uint64_t m2) { return cid::fold_factor(m, m2); }
// writes at most cap divisors of m (ascending) to out; returns how many there are
uint64_t shim_divisors_of(uint64_t m, uint64_t *out, uint64_t cap) {
    const std::vector<uint64_t> d = cid::divisors_of(m);
    for (uint64_t i = 0; i < d.size() && i < cap; ++i) out[i] = d[i];
    return d.size();
}
void shim_nearest_divisors(uint64_t m, uint64_t s, uint64_t *below, uint64_t *above) { cid::nearest_divisors(m, s, *below, *above); }

}  // extern "C"
