// ristretto255_dev.h -- the ristretto255 prime-order group (RFC 9496) on gfx950, one element per lane, with hash-to-group and
// hash-to-scalar (RFC 9380 expand_message_xmd over SHA-512).
//
// Replaces group/ristretto255.go (which hands the point arithmetic to an outside package) for batch work.  Written from RFC 9496
// section 4 on the project's own arithmetic: GF(2^255 - 19) of x25519_dev.h, the extended-coordinate points, the fixed-base comb and
// the scalars mod L of ed25519_dev.h, SHA-512 through the run-time-length streams of hkdf_stream_dev.h.
//
//   sqrt_ratio_m1     4.2: one (p - 5) / 8 power, three comparisons on canonical words, selects; no branch
//   r255_decode       4.3.1, STRICT: s >= p, a negative s, a non-square, a negative t and y = 0 all give verdict 0.  The reference
//                     reduces s >= p and ignores bit 255; here both are rejected.  Computes either way, like ge_decode.
//   r255_encode       4.3.2: one sqrt_ratio_m1, no inversion
//   r255_map          4.3.4 (Elligator).  SQRT_AD_MINUS_ONE is the ODD root of a d - 1, as the RFC lists it; every other constant is
//                     the even one.
//   r255_mul          k P for a SECRET k and a SECRET P: double-and-add-always from the top bit, the addend chosen between P and the
//                     neutral element by per-lane selects on the bit.  No table, so nothing secret is ever addressed or stored; no
//                     branch or address depends on k or P (DESIGN.md 4.8f weighs it against a masked radix-16 table).
//   sc_mul / sc_inv   products mod L through sc_muladd; x^(L - 2) by square-and-multiply over the PUBLIC exponent (its bits steer
//                     wave-uniform branches), 252 squarings and 65 products for every x.  0 maps to 0: the caller masks it.
//   (hashing)         expand_message_xmd is hkdf::xmd<hkdf::Sha512, WV>(out, 64, ...) of hkdf_stream_dev.h: exactly one b_1.
#pragma once
#include <stdint.h>

#include "ed25519_dev.h"
#include "hkdf_stream_dev.h"

namespace circl {
namespace r255 {

using ed25519::fe_carry;
using ed25519::fe_lit;
using ed25519::fe_neg;
using ed25519::fe_select;
using ed25519::Ge;
using ed25519::GeCached;
using x25519::Fe;
using x25519::fe_add;
using x25519::fe_const;
using x25519::fe_mul;
using x25519::fe_sqr;
using x25519::fe_sub;
using x25519::fe_to_words;

// ---- constants of RFC 9496 4.1 (limbs of x25519_dev.h) -----------------------------------------------------------------------
CIRCL_HD Fe fe_sqrt_ad_minus_one() {  // the odd root
    constexpr uint32_t l[10] = {0x17b2e1bu, 0x1fda812u, 0x297afd2u, 0x60dbc2u, 0x2be7638u, 0x1f5d1fdu, 0x27e6498u, 0x11581e7u, 0x3f2b834u, 0xdda4c6u};
    return fe_lit(l);
}
CIRCL_HD Fe fe_invsqrt_a_minus_d() {
    constexpr uint32_t l[10] = {0x5d40eau, 0x3f6aa0u, 0x257d339u, 0xbad20bu, 0x274bc58u, 0x1d840u, 0x13dc8ffu, 0x19442d8u, 0x5cfaffu, 0x1e1b224u};
    return fe_lit(l);
}
CIRCL_HD Fe fe_one_minus_d_sq() {
    constexpr uint32_t l[10] = {0x5fc176u, 0x1027065u, 0x2a1fc4fu, 0x1c66af1u, 0xb20684u, 0x70dfe4u, 0x255eedfu, 0x1af332u, 0x28b2b3eu, 0xa41cau};
    return fe_lit(l);
}
CIRCL_HD Fe fe_d_minus_one_sq() {
    constexpr uint32_t l[10] = {0xed4d20u, 0x156aa91u, 0x3332635u, 0x16580f0u, 0x34a7928u, 0x9b4eebu, 0x26997a9u, 0x48299bu, 0x3af66c2u, 0x165a2cdu};
    return fe_lit(l);
}

// ---- field helpers: every result is "carried" (x25519_dev.h), so that it may go anywhere ---------------------------------------
CIRCL_HD Fe fe_addc(const Fe &a, const Fe &b) { return fe_carry(fe_add(a, b)); }
CIRCL_HD Fe fe_subc(const Fe &a, const Fe &b) { return fe_carry(fe_sub(a, b)); }  // b carried
CIRCL_HD Fe fe_negc(const Fe &a) { return fe_carry(fe_neg(a)); }                  // a carried
CIRCL_HD bool fe_is_negative(const Fe &a) {  // the low bit of the canonical value (a carried)
    uint32_t w[8];
    fe_to_words(w, a);
    return (w[0] & 1u) != 0;
}
CIRCL_HD bool fe_is_zero(const Fe &a) {
    uint32_t w[8], o = 0;
    fe_to_words(w, a);
#pragma unroll
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}
CIRCL_HD bool fe_equal(const Fe &a, const Fe &b) {
    uint32_t x[8], y[8];
    fe_to_words(x, a);
    fe_to_words(y, b);
    return ed25519::words_equal(x, y);
}
CIRCL_HD Fe fe_abs(const Fe &a) { return fe_select(a, fe_negc(a), fe_is_negative(a)); }  // a carried

// RFC 9496 4.2 SQRT_RATIO_M1(u, v): was_square and the non-negative root of u / v, or of SQRT_M1 u / v for a non-square; (true, 0) for
// u = 0, (false, 0) for v = 0 and u != 0.  u and v carried.
CIRCL_HD bool sqrt_ratio_m1(Fe &root, const Fe &u, const Fe &v) {
    const Fe v3 = fe_mul(fe_sqr(v), v);
    const Fe v7 = fe_mul(fe_sqr(v3), v);
    Fe r = fe_mul(fe_mul(u, v3), ed25519::fe_pow22523(fe_mul(u, v7)));
    const Fe check = fe_mul(v, fe_sqr(r));
    const Fe nu = fe_negc(u);
    const bool correct = fe_equal(check, u), flipped = fe_equal(check, nu), flipped_i = fe_equal(check, fe_mul(nu, ed25519::fe_sqrtm1()));
    r = fe_select(r, fe_mul(r, ed25519::fe_sqrtm1()), flipped || flipped_i);
    root = fe_abs(r);
    return correct || flipped;
}

// ---- elements ----------------------------------------------------------------------------------------------------------------
// RFC 9496 4.3.1: 1 and the point (every coordinate carried, Z = 1), or 0; the point is computed either way
CIRCL_HD uint32_t r255_decode(Ge &p, const uint32_t in[8]) {
    bool ge_p = in[7] == 0x7fffffffu && in[0] >= 0xffffffedu;  // s >= p = 2^255 - 19 with bit 255 clear ...
#pragma unroll
    for (int i = 1; i < 7; i++) ge_p = ge_p && in[i] == 0xffffffffu;
    ge_p = ge_p || (in[7] >> 31) != 0;  // ... or bit 255 set
    const bool s_neg = (in[0] & 1u) != 0;
    const Fe s = x25519::fe_from_words(in);
    const Fe one = fe_const(1);
    const Fe ss = fe_sqr(s);
    const Fe u1 = fe_subc(one, ss), u2 = fe_addc(one, ss);
    const Fe u2_sqr = fe_sqr(u2);
    const Fe v = fe_subc(fe_negc(fe_mul(ed25519::fe_d(), fe_sqr(u1))), u2_sqr);  // -(d u1^2) - u2^2
    Fe invsqrt;
    const bool was_square = sqrt_ratio_m1(invsqrt, one, fe_mul(v, u2_sqr));
    const Fe den_x = fe_mul(invsqrt, u2);
    const Fe den_y = fe_mul(fe_mul(invsqrt, den_x), v);
    const Fe x = fe_abs(fe_mul(fe_addc(s, s), den_x));
    const Fe y = fe_mul(u1, den_y);
    const Fe t = fe_mul(x, y);
    p.X = x;
    p.Y = y;
    p.Z = one;
    p.T = t;
    return (!ge_p && !s_neg && was_square && !fe_is_negative(t) && !fe_is_zero(y)) ? 1u : 0u;
}

// RFC 9496 4.3.2: the canonical encoding (eight little-endian words) of a point with carried coordinates
CIRCL_HD void r255_encode(uint32_t out[8], const Ge &p) {
    const Fe u1 = fe_mul(fe_addc(p.Z, p.Y), fe_subc(p.Z, p.Y));
    const Fe u2 = fe_mul(p.X, p.Y);
    Fe invsqrt;
    (void)sqrt_ratio_m1(invsqrt, fe_const(1), fe_mul(u1, fe_sqr(u2)));
    const Fe den1 = fe_mul(invsqrt, u1), den2 = fe_mul(invsqrt, u2);
    const Fe z_inv = fe_mul(fe_mul(den1, den2), p.T);
    const Fe ix0 = fe_mul(p.X, ed25519::fe_sqrtm1()), iy0 = fe_mul(p.Y, ed25519::fe_sqrtm1());
    const Fe enchanted = fe_mul(den1, fe_invsqrt_a_minus_d());
    const bool rotate = fe_is_negative(fe_mul(p.T, z_inv));
    const Fe x = fe_select(p.X, iy0, rotate);
    Fe y = fe_select(p.Y, ix0, rotate);
    const Fe den_inv = fe_select(den2, enchanted, rotate);
    y = fe_select(y, fe_negc(y), fe_is_negative(fe_mul(x, z_inv)));
    fe_to_words(out, fe_abs(fe_mul(den_inv, fe_subc(p.Z, y))));
}

// RFC 9496 4.5 on encodings: the identity is the element whose canonical encoding is 32 zero bytes
CIRCL_HD bool r255_equal_identity(const uint32_t enc[8]) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= enc[i];
    return o == 0;
}

// RFC 9496 4.3.4 MAP on 255 bits (eight words; bit 255 is masked here)
CIRCL_HD Ge r255_map(const uint32_t tw[8]) {
    uint32_t m[8];
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = tw[i];
    m[7] &= 0x7fffffffu;
    const Fe t = x25519::fe_from_words(m);
    const Fe one = fe_const(1), d = ed25519::fe_d();
    const Fe r = fe_mul(ed25519::fe_sqrtm1(), fe_sqr(t));
    const Fe u = fe_mul(fe_addc(r, one), fe_one_minus_d_sq());
    const Fe minus_one = fe_negc(one);
    const Fe v = fe_mul(fe_subc(minus_one, fe_mul(r, d)), fe_addc(r, d));
    Fe s;
    const bool was_square = sqrt_ratio_m1(s, u, v);
    const Fe s_prime = fe_negc(fe_abs(fe_mul(s, t)));
    s = fe_select(s, s_prime, !was_square);
    const Fe c = fe_select(minus_one, r, !was_square);
    const Fe N = fe_subc(fe_mul(fe_mul(c, fe_subc(r, one)), fe_d_minus_one_sq()), v);
    const Fe ss = fe_sqr(s);
    const Fe w0 = fe_mul(fe_addc(s, s), v), w1 = fe_mul(N, fe_sqrt_ad_minus_one()), w2 = fe_subc(one, ss), w3 = fe_addc(one, ss);
    return {fe_mul(w0, w3), fe_mul(w2, w1), fe_mul(w1, w3), fe_mul(w0, w2)};
}

// k P for k below 2^253, k and P secret: 253 doublings and 253 additions of P or of the neutral element (cached: (1, 1, 0, 2)),
// chosen by selects.  The sum with the neutral element is the same point in other projective coordinates.
CIRCL_HD Ge r255_mul(const uint32_t k_in[8], const Ge &p) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = k_in[i];
    // bit 252 first: shifted left by three so that the current bit is always the top bit of k[7]
#pragma unroll
    for (int i = 7; i > 0; i--) k[i] = (k[i] << 3) | (k[i - 1] >> 29);
    k[0] <<= 3;
    const GeCached q = ed25519::ge_to_cached(p), e = ed25519::ge_cached_identity();
    Ge r = ed25519::ge_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 252; t >= 0; t--) {
        const bool bit = (k[7] >> 31) != 0;
#pragma unroll
        for (int i = 7; i > 0; i--) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
        k[0] <<= 1;
        const GeCached a = {fe_select(e.YpX, q.YpX, bit), fe_select(e.YmX, q.YmX, bit), fe_select(e.T2d, q.T2d, bit), fe_select(e.Z2, q.Z2, bit)};
        r = ed25519::ge_add(ed25519::ge_dbl(r), a, false);
    }
    return r;
}

// k B through the comb (k below 2^255)
CIRCL_HD Ge r255_base(const uint32_t k[8]) { return ed25519::ge_base(k); }

CIRCL_HD Ge r255_add(const Ge &p, const Ge &q) { return ed25519::ge_add(p, ed25519::ge_to_cached(q), false); }

// ---- scalars -----------------------------------------------------------------------------------------------------------------
CIRCL_HD void sc_mul(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ed25519::sc_muladd(out, a, b, zero);
}
CIRCL_HD bool sc_is_zero(const uint32_t s[8]) { return r255_equal_identity(s); }

// x^(L - 2) mod L for x below L: from the top bit of the public exponent, a squaring per bit and a product where the bit is set
CIRCL_HD void sc_inv(uint32_t out[8], const uint32_t x[8]) {
    uint32_t r[8];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = x[i];  // bit 252 of L - 2
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 251; t >= 0; t--) {
        uint32_t sq[8];
        sc_mul(sq, r, r);
        const uint32_t ew = ed25519::order_word(t >> 5) - (t < 32 ? 2u : 0u);  // L - 2: the low word of L ends in ...ed, no borrow
        if ((ew >> (t & 31)) & 1u) sc_mul(r, sq, x);
        else {
#pragma unroll
            for (int i = 0; i < 8; i++) r[i] = sq[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = r[i];
}

// ---- hashing -----------------------------------------------------------------------------------------------------------------
// group.Ristretto255.HashToElement on the 64 uniform bytes: each half masked to 255 bits and mapped, the two points added
CIRCL_HD Ge r255_from_uniform(const uint32_t u[16]) { return r255_add(r255_map(u), r255_map(u + 8)); }

// group.Ristretto255.HashToScalar on the 64 uniform bytes: the little-endian value mod L
CIRCL_HD void sc_from_uniform(uint32_t out[8], const uint32_t u[16]) { ed25519::sc_reduce(out, u); }

}  // namespace r255
}  // namespace circl
