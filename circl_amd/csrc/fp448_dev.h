// fp448_dev.h -- GF(p), p = 2^448 - 2^224 - 1 (the Goldilocks prime), on gfx950: one field element per lane.
//
// Replaces math/fp448 (fp.go, fp_generic.go and the ADX/BMI2 assembler) under dh/x448, ecc/goldilocks and sign/ed448.
//
// Sixteen limbs of 28 bits in 32-bit registers, 64-bit column sums from V_MAD_U64_U32, as x25519_dev.h does for 2^255 - 19.
// With phi = 2^224 (eight limbs) the prime is phi^2 - phi - 1, so a product is one level of Karatsuba:
//     (a0 + a1 phi)(b0 + b1 phi) = (a0 b0 + a1 b1) + phi ((a0 + a1)(b0 + b1) - a0 b0)        (phi^2 = phi + 1)
// three 8 x 8 limb products (192 multiply-accumulates, 108 for a square) whose upper halves wrap by the same rule; every
// column of the result is a sum of non-negative limb products (at most 38 of them), accumulated modulo 2^64 -- the one
// subtraction is exact there.  Everything is unsigned.  Bounds (C = 2^28 + 2^9):
//     "carried" (output of mul / sqr / mul_small / carry / sub / neg):  limbs < C
//     sum of two carried values (fe_add):                               limbs < 2 C
//     difference (fe_sub: a + 2p - b, then ONE parallel carry step):    limbs < 2^28 + 2^5 for a < 2^31, b < 2^29 - 4
// so a difference is as good as a carried value and needs no second pass.  fe_mul / fe_sqr need
// 38 (bound of a) (bound of b) < 2^64: any two sums of two carried values (2^63.3), or a sum of four with a carried value.
// tests/test_curve448_hostsim.py drives the host instantiation with every limb at these bounds.
#pragma once
#include <stdint.h>

#ifndef CIRCL_HD
#if defined(__HIPCC__)
#define CIRCL_HD __host__ __device__ __forceinline__
#else
#define CIRCL_HD inline
#endif
#endif

namespace circl {
namespace fp448 {

struct Fe {
    uint32_t v[16];
};

constexpr uint32_t M28 = (1u << 28) - 1;
// limbs of p: all 2^28 - 1 except limb 8 (2^28 - 2)
CIRCL_HD constexpr uint32_t p_limb(int i) { return i == 8 ? M28 - 1 : M28; }

CIRCL_HD Fe fe_const(uint32_t c) {  // c < 2^28
    Fe r;
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = 0;
    r.v[0] = c;
    return r;
}

// 448-bit little-endian value in fourteen words -> limbs (any value below 2^448; not reduced)
CIRCL_HD Fe fe_from_words(const uint32_t w[14]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int pos = 28 * i, k = pos >> 5, s = pos & 31;
        uint32_t x = w[k] >> s;
        if (s > 4) x |= w[k + 1] << (32 - s);
        r.v[i] = x & M28;
    }
    return r;
}

// one carry chain over 64-bit column sums below 2^63.9: h0 -> h1 -> ... -> h15 -> (2^448 = 2^224 + 1) limbs 0 and 8
CIRCL_HD Fe fe_carry64(uint64_t h[16]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 15; i++) {
        h[i + 1] += h[i] >> 28;
        r.v[i] = (uint32_t)h[i] & M28;
    }
    const uint64_t c = h[15] >> 28;  // < 2^36
    r.v[15] = (uint32_t)h[15] & M28;
    const uint64_t t0 = (uint64_t)r.v[0] + c, t8 = (uint64_t)r.v[8] + c;
    r.v[0] = (uint32_t)t0 & M28;
    r.v[1] += (uint32_t)(t0 >> 28);  // < 2^9
    r.v[8] = (uint32_t)t8 & M28;
    r.v[9] += (uint32_t)(t8 >> 28);
    return r;
}

CIRCL_HD Fe fe_carry(const Fe &a) {  // limbs below 2^32 -> carried
    uint64_t h[16];
#pragma unroll
    for (int i = 0; i < 16; i++) h[i] = a.v[i];
    return fe_carry64(h);
}

CIRCL_HD Fe fe_add(const Fe &a, const Fe &b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = a.v[i] + b.v[i];
    return r;
}

// a - b: t = a + 2p - b limb-wise (a < 2^31, b < 2^29 - 4, so carried), then every limb hands its bits above 28 to the next one
// at once (the top limb to limbs 0 and 8): the result's limbs are below 2^28 + 2^5
CIRCL_HD Fe fe_sub(const Fe &a, const Fe &b) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = a.v[i] + 2 * p_limb(i) - b.v[i];
    Fe r;
    const uint32_t top = t[15] >> 28;
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = (t[i] & M28) + (i ? t[i - 1] >> 28 : top) + (i == 8 ? top : 0u);
    return r;
}
CIRCL_HD Fe fe_neg(const Fe &a) { return fe_sub(fe_const(0), a); }

// (a0 + a1 phi)(b0 + b1 phi) mod p into sixteen column sums.  z0 = a0 b0, z2 = a1 b1, z1 = (a0 + a1)(b0 + b1), fifteen columns
// each; column 8 + j of a half product is phi times column j.  With X = z0 + z2 and Y = z1 - z0:
//     low half  h[j]     = X[j] + Y[8 + j]            = z0[j] - z0[8 + j] + z2[j] + z1[8 + j]
//     high half h[8 + j] = X[8 + j] + Y[j] + Y[8 + j] = -z0[j] + z2[8 + j] + z1[j] + z1[8 + j]
CIRCL_HD Fe fe_mul(const Fe &a, const Fe &b) {
    uint64_t z0[15];
#pragma unroll
    for (int k = 0; k < 15; k++) z0[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) z0[i + j] += (uint64_t)a.v[i] * b.v[j];
    uint64_t h[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        h[j] = z0[j] - (j < 7 ? z0[8 + j] : 0);
        h[8 + j] = 0 - z0[j];
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) h[i + j] += (uint64_t)a.v[8 + i] * b.v[8 + j];  // z2: column s -> h[s]
    uint32_t sa[8], sb[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        sa[i] = a.v[i] + a.v[8 + i];
        sb[i] = b.v[i] + b.v[8 + i];
    }
    uint64_t z1h[7];
#pragma unroll
    for (int k = 0; k < 7; k++) z1h[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t t = (uint64_t)sa[i] * sb[j];
            if (i + j < 8) h[8 + i + j] += t;
            else z1h[i + j - 8] += t;
        }
#pragma unroll
    for (int k = 0; k < 7; k++) {
        h[k] += z1h[k];
        h[8 + k] += z1h[k];
    }
    return fe_carry64(h);
}

// the same with the symmetric terms taken once against a doubled operand (108 multiply-accumulates)
CIRCL_HD Fe fe_sqr(const Fe &a) {
    uint32_t a2[16], sa[8], sa2[8];
#pragma unroll
    for (int i = 0; i < 16; i++) a2[i] = a.v[i] << 1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        sa[i] = a.v[i] + a.v[8 + i];
        sa2[i] = sa[i] << 1;
    }
    uint64_t z0[15];
#pragma unroll
    for (int k = 0; k < 15; k++) z0[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++) z0[i + j] += (uint64_t)(i < j ? a2[i] : a.v[i]) * a.v[j];
    uint64_t h[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        h[j] = z0[j] - (j < 7 ? z0[8 + j] : 0);
        h[8 + j] = 0 - z0[j];
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++) h[i + j] += (uint64_t)(i < j ? a2[8 + i] : a.v[8 + i]) * a.v[8 + j];
    uint64_t z1h[7];
#pragma unroll
    for (int k = 0; k < 7; k++) z1h[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++) {
            const uint64_t t = (uint64_t)(i < j ? sa2[i] : sa[i]) * sa[j];
            if (i + j < 8) h[8 + i + j] += t;
            else z1h[i + j - 8] += t;
        }
#pragma unroll
    for (int k = 0; k < 7; k++) {
        h[k] += z1h[k];
        h[8 + k] += z1h[k];
    }
    return fe_carry64(h);
}

// f * c for a small constant (c < 2^20; 39081 and 156326 are what the curves need), f's limbs below 2^32
CIRCL_HD Fe fe_mul_small(const Fe &f, uint32_t c) {
    uint64_t h[16];
#pragma unroll
    for (int i = 0; i < 16; i++) h[i] = (uint64_t)f.v[i] * c;
    return fe_carry64(h);
}

// per-lane select on the bit (two V_CNDMASK per limb on the device; no branch)
CIRCL_HD void fe_cswap(Fe &a, Fe &b, uint32_t bit) {
    const bool c = bit != 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t ta = a.v[i], tb = b.v[i];
        a.v[i] = c ? tb : ta;
        b.v[i] = c ? ta : tb;
    }
}
CIRCL_HD Fe fe_select(const Fe &a, const Fe &b, bool take_b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 16; i++) r.v[i] = take_b ? b.v[i] : a.v[i];
    return r;
}

CIRCL_HD Fe fe_sqr_n(Fe t, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < n; i++) t = fe_sqr(t);
    return t;
}

// z^((p-3)/4) = z^(2^446 - 2^222 - 1) = (z^(2^223 - 1))^(2^223) z^(2^222 - 1): 445 squarings, 12 products
CIRCL_HD Fe fe_pow_p34(const Fe &z) {
    const Fe x2 = fe_mul(fe_sqr(z), z);
    const Fe x3 = fe_mul(fe_sqr(x2), z);
    const Fe x6 = fe_mul(fe_sqr_n(x3, 3), x3);
    const Fe x9 = fe_mul(fe_sqr_n(x6, 3), x3);
    const Fe x18 = fe_mul(fe_sqr_n(x9, 9), x9);
    const Fe x19 = fe_mul(fe_sqr(x18), z);
    const Fe x37 = fe_mul(fe_sqr_n(x19, 18), x18);
    const Fe x74 = fe_mul(fe_sqr_n(x37, 37), x37);
    const Fe x111 = fe_mul(fe_sqr_n(x74, 37), x37);
    const Fe x222 = fe_mul(fe_sqr_n(x111, 111), x111);
    const Fe x223 = fe_mul(fe_sqr(x222), z);
    return fe_mul(fe_sqr_n(x223, 223), x222);
}

// z^(p-2) = (z^((p-3)/4))^4 z; 0 for z = 0
CIRCL_HD Fe fe_inv(const Fe &z) { return fe_mul(fe_sqr_n(fe_pow_p34(z), 2), z); }

// the canonical value (below p) of an element with limbs below 2^31, as fourteen little-endian words (fp.go ToBytes / Modp)
CIRCL_HD void fe_to_words(uint32_t w[14], const Fe &a) {
    uint32_t l[16];
#pragma unroll
    for (int i = 0; i < 16; i++) l[i] = a.v[i];
    // two strict passes: after the first the value is below 2^448 + 2^229, after the second below 2^448 with every limb strict
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
#pragma unroll
        for (int i = 0; i < 15; i++) {
            l[i + 1] += l[i] >> 28;
            l[i] &= M28;
        }
        const uint32_t c = l[15] >> 28;
        l[15] &= M28;
        l[0] += c;
        l[8] += c;
    }
    // q = 1 iff the value is >= p, i.e. iff value + 2^224 + 1 carries out of bit 448
    uint32_t q = (l[0] + 1) >> 28;
#pragma unroll
    for (int i = 1; i < 16; i++) q = (l[i] + q + (i == 8 ? 1u : 0u)) >> 28;
    l[0] += q;
    l[8] += q;
#pragma unroll
    for (int i = 0; i < 15; i++) {
        l[i + 1] += l[i] >> 28;
        l[i] &= M28;
    }
    l[15] &= M28;
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const int i = (32 * k) / 28, s = 32 * k - 28 * i;  // word k starts at bit s of limb i
        uint32_t x = l[i] >> s;
        x |= l[i + 1] << (28 - s);  // s is a multiple of 4 up to 24: two limbs always cover the word
        w[k] = x;
    }
}

CIRCL_HD bool fe_is_zero(const Fe &a) {
    uint32_t w[14], o = 0;
    fe_to_words(w, a);
#pragma unroll
    for (int i = 0; i < 14; i++) o |= w[i];
    return o == 0;
}

// x = sqrt(u / v) and true when u / v is a square (the reference's fp.InvSqrt); u, v carried.  x = u^3 v (u^5 v^3)^((p-3)/4),
// whose square is +-u / v: the flag is v x^2 == u.  u = 0 gives x = 0 and true.
CIRCL_HD bool fe_sqrt_ratio(Fe &x, const Fe &u, const Fe &v) {
    const Fe u2 = fe_sqr(u), u3v = fe_mul(fe_mul(u2, u), v);
    const Fe u5v3 = fe_mul(fe_mul(u3v, u2), fe_sqr(v));
    x = fe_mul(u3v, fe_pow_p34(u5v3));
    return fe_is_zero(fe_sub(fe_mul(v, fe_sqr(x)), u));
}

}  // namespace fp448
}  // namespace circl
