// tests/hostsim/x448_comb_hostsim.hip -- TEST INFRASTRUCTURE: runs the two X448 KeyGen routes of circl_amd/csrc/x448_dev.h on the
// CPU (their host instantiation), so that the CPU-only test tier can check the fixed-base comb against the ladder and against
// tests/curve448.py.  Nothing here is linked into libcirclhip.so.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "x448_dev.h"

using namespace circl;

extern "C" {

// X448(k, 5) by the Ed448 comb and the isogeny u = y^2 / x^2
void hs_x448_base_comb(uint32_t *out, const uint32_t *k) { x448::base_mult_comb(out, k); }
// X448(k, 5) by the ladder
void hs_x448_base_ladder(uint32_t *out, const uint32_t *k) { x448::scalar_mult<true>(out, k, nullptr); }

}  // extern "C"
