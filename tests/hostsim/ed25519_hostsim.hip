// tests/hostsim/ed25519_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/sha512_dev.h and ed25519_dev.h on the CPU (their host instantiation), so that the CPU-only test tier can
// check the very source the Ed25519 kernels are built from against tests/ed25519.py and hashlib.  Nothing here is linked
// into libcirclhip.so.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "ed25519_dev.h"

using namespace circl;

namespace {
void to_fe(ed25519::Fe &f, const uint32_t *l) {
    for (int i = 0; i < 10; i++) f.v[i] = l[i];
}
void from_fe(uint32_t *l, const ed25519::Fe &f) {
    for (int i = 0; i < 10; i++) l[i] = f.v[i];
}
}  // namespace

extern "C" {

// SHA-512(head || msg): head_words in {0, 8, 16}
void hs_sha512(uint32_t *out, const uint32_t *head, int head_words, const uint8_t *msg, uint64_t len) {
    if (head_words == 16) sha512::hash<16>(out, head, msg, len);
    else if (head_words == 8) sha512::hash<8>(out, head, msg, len);
    else sha512::hash<0>(out, nullptr, msg, len);
}

void hs_sc_reduce(uint32_t *out, const uint32_t *x) { ed25519::sc_reduce(out, x); }
void hs_sc_muladd(uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c) { ed25519::sc_muladd(out, a, b, c); }
uint32_t hs_sc_is_canonical(const uint32_t *s) { return ed25519::sc_is_canonical(s); }

// decode, then re-encode what was decoded
uint32_t hs_decode(uint32_t *enc, const uint32_t *in) {
    ed25519::Ge p;
    const uint32_t ok = ed25519::ge_decode(p, in);
    ed25519::ge_encode(enc, p);
    return ok;
}

// enc(k B) through the comb of x25519_dev.h (k below 2^255)
void hs_base(uint32_t *out, const uint32_t *k) { ed25519::ge_encode(out, ed25519::ge_base(k)); }

// enc([s]B + [k](-A)): the table in a local buffer (stride 1), then the joint multiplication of the verify kernel
uint32_t hs_double_scalar(uint32_t *out, const uint32_t *s, const uint32_t *k, const uint32_t *pk) {
    uint32_t tab[8 * 40];
    ed25519::Ge a;
    const uint32_t ok = ed25519::ge_decode(a, pk);
    a.X = ed25519::fe_carry(ed25519::fe_neg(a.X));
    a.T = ed25519::fe_carry(ed25519::fe_neg(a.T));
    ed25519::table_build(tab, 1, 0, a);
    ed25519::ge_encode(out, ed25519::double_scalar_mult(s, k, tab, 1, 0));
    return ok;
}

// the point formulas on raw limbs (p, q: X, Y, Z, T / Y+X, Y-X, 2dT, 2Z as 4 x 10 limbs)
void hs_ge_dbl(uint32_t *out, const uint32_t *p) {
    ed25519::Ge a;
    to_fe(a.X, p), to_fe(a.Y, p + 10), to_fe(a.Z, p + 20), to_fe(a.T, p + 30);
    const ed25519::Ge r = ed25519::ge_dbl(a);
    from_fe(out, r.X), from_fe(out + 10, r.Y), from_fe(out + 20, r.Z), from_fe(out + 30, r.T);
}
void hs_ge_add(uint32_t *out, const uint32_t *p, const uint32_t *q, int neg) {
    ed25519::Ge a;
    ed25519::GeCached c;
    to_fe(a.X, p), to_fe(a.Y, p + 10), to_fe(a.Z, p + 20), to_fe(a.T, p + 30);
    to_fe(c.YpX, q), to_fe(c.YmX, q + 10), to_fe(c.T2d, q + 20), to_fe(c.Z2, q + 30);
    const ed25519::Ge r = ed25519::ge_add(a, c, neg != 0);
    from_fe(out, r.X), from_fe(out + 10, r.Y), from_fe(out + 20, r.Z), from_fe(out + 30, r.T);
}

}  // extern "C"
