// tests/hostsim/curve448_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/fp448_dev.h, x448_dev.h and ed448_dev.h on the CPU (their host instantiation), so that the CPU-only test tier
// can check the very source the Curve448 kernels are built from against tests/curve448.py and Python integers.  Nothing here is
// linked into libcirclhip.so.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "ed448_dev.h"
#include "x448_dev.h"

using namespace circl;
using fp448::Fe;

namespace {
Fe to_fe(const uint32_t *l) {
    Fe f;
    for (int i = 0; i < 16; i++) f.v[i] = l[i];
    return f;
}
void from_fe(uint32_t *l, const Fe &f) {
    for (int i = 0; i < 16; i++) l[i] = f.v[i];
}
ed448::Ge to_ge(const uint32_t *p) { return {to_fe(p), to_fe(p + 16), to_fe(p + 32), to_fe(p + 48)}; }
void from_ge(uint32_t *o, const ed448::Ge &r) { from_fe(o, r.X), from_fe(o + 16, r.Y), from_fe(o + 32, r.Z), from_fe(o + 48, r.T); }
}  // namespace

extern "C" {

// ---- the field, on raw limbs ----
void hs_fe_mul(uint32_t *out, const uint32_t *a, const uint32_t *b) { from_fe(out, fp448::fe_mul(to_fe(a), to_fe(b))); }
void hs_fe_sqr(uint32_t *out, const uint32_t *a) { from_fe(out, fp448::fe_sqr(to_fe(a))); }
void hs_fe_sub(uint32_t *out, const uint32_t *a, const uint32_t *b) { from_fe(out, fp448::fe_sub(to_fe(a), to_fe(b))); }
void hs_fe_mul_small(uint32_t *out, const uint32_t *a, uint32_t c) { from_fe(out, fp448::fe_mul_small(to_fe(a), c)); }
void hs_fe_carry(uint32_t *out, const uint32_t *a) { from_fe(out, fp448::fe_carry(to_fe(a))); }
void hs_fe_from_words(uint32_t *out, const uint32_t *w) { from_fe(out, fp448::fe_from_words(w)); }
void hs_fe_to_words(uint32_t *w, const uint32_t *a) { fp448::fe_to_words(w, to_fe(a)); }
void hs_fe_inv(uint32_t *w, const uint32_t *a) { fp448::fe_to_words(w, fp448::fe_inv(to_fe(a))); }
uint32_t hs_fe_sqrt_ratio(uint32_t *w, const uint32_t *u, const uint32_t *v) {
    Fe x;
    const bool sq = fp448::fe_sqrt_ratio(x, to_fe(u), to_fe(v));
    fp448::fe_to_words(w, x);
    return sq ? 1u : 0u;
}

// ---- X448 ----
uint32_t hs_x448(uint32_t *out, const uint32_t *k, const uint32_t *u) {
    if (u) x448::scalar_mult<false>(out, k, u);
    else x448::scalar_mult<true>(out, k, nullptr);
    return u ? x448::valid_public(u) : 1u;
}

// ---- scalars ----
void hs_sc_reduce(uint32_t *out, const uint32_t *x) { ed448::sc_reduce(out, x); }
void hs_sc_reduce_small(uint32_t *out, const uint32_t *x) { ed448::sc_reduce_small(out, x); }
void hs_sc_muladd(uint32_t *out, const uint32_t *a, const uint32_t *b, const uint32_t *c) { ed448::sc_muladd(out, a, b, c); }
void hs_sc_div4(uint32_t *out, const uint32_t *x) { ed448::sc_div4(out, x); }
uint32_t hs_sc_is_canonical(const uint32_t *s) { return ed448::sc_is_canonical(s); }

// ---- bytes and SHAKE256 ----
uint32_t hs_bytes_word(const uint8_t *p, uint64_t len, int64_t q) { return ed448::bytes_word(p, len, q); }
// SHAKE256([dom4(ctx) ||] mid || msg, 114); mid_words in {15, 29}
void hs_shake(uint32_t *out, int dom, const uint8_t *ctx, uint32_t clen, const uint32_t *mid, int mid_words, uint32_t mid_bytes, const uint8_t *msg,
              uint64_t mlen) {
    uint32_t m15[15], m29[29];
    for (int i = 0; i < 15; i++) m15[i] = i < mid_words ? mid[i] : 0;
    for (int i = 0; i < 29; i++) m29[i] = i < mid_words ? mid[i] : 0;
    if (mid_words == 15) {
        if (dom) ed448::shake256_114<true, 15>(out, ctx, clen, m15, mid_bytes, msg, mlen);
        else ed448::shake256_114<false, 15>(out, ctx, clen, m15, mid_bytes, msg, mlen);
    } else {
        if (dom) ed448::shake256_114<true, 29>(out, ctx, clen, m29, mid_bytes, msg, mlen);
        else ed448::shake256_114<false, 29>(out, ctx, clen, m29, mid_bytes, msg, mlen);
    }
}

// ---- points ----
// decode, then re-encode what was decoded
uint32_t hs_decode(uint32_t *enc, const uint32_t *in) {
    ed448::Ge p;
    const uint32_t ok = ed448::ge_decode(p, in);
    ed448::ge_encode(enc, p);
    return ok;
}
// enc(k B) through the fixed-base routine (k below 2^446)
void hs_base(uint32_t *out, const uint32_t *k) { ed448::ge_encode(out, ed448::ge_base(k)); }

// -A's table in a local buffer (stride 1), then enc([s]B + [k](-A)) (combined = 0) or enc(CombinedMult(s, k, -A)) with both
// scalars divided by 4 first, as the verify kernels do (combined = 1)
uint32_t hs_double_scalar(uint32_t *out, const uint32_t *s, const uint32_t *k, const uint32_t *pk, int combined) {
    static uint32_t tab[ed448::kTableWords], rec[ed448::kRecodedWords];
    ed448::Ge a;
    const uint32_t ok = ed448::ge_decode(a, pk);
    a.X = fp448::fe_neg(a.X);
    a.T = fp448::fe_neg(a.T);
    ed448::table_build(tab, 1, 0, a);
    if (combined) {
        ed448::recode_store_div4(rec, 1, 0, 0, s);
        ed448::recode_store_div4(rec, 1, 0, 1, k);
        ed448::ge_encode(out, ed448::combined_mult(rec, tab, 1, 0));
    } else {
        ed448::recode_prepare(rec, s);
        ed448::recode_prepare(rec + 14, k);
        ed448::ge_encode(out, ed448::double_scalar_mult(rec, tab, 1, 0));
    }
    return ok;
}

// the point formulas on raw limbs (p: X, Y, Z, T; q: X, Y, Z, 39081 T as 4 x 16 limbs)
void hs_ge_dbl(uint32_t *out, const uint32_t *p) { from_ge(out, ed448::ge_dbl(to_ge(p), true)); }
void hs_ge_add(uint32_t *out, const uint32_t *p, const uint32_t *q, int neg) {
    const ed448::GeCached c = {to_fe(q), to_fe(q + 16), to_fe(q + 32), to_fe(q + 48)};
    from_ge(out, ed448::ge_add(to_ge(p), c, neg != 0));
}

}  // extern "C"
