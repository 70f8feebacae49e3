// ed25519_dev.h -- Ed25519 (RFC 8032 5.1, pure) on gfx950, one key / signature per lane.
//
// Replaces sign/ed25519 (ed25519.go, point.go, modular.go, mult.go) for batch key generation, signing and verification.
// Built on the GF(2^255 - 19) arithmetic of x25519_dev.h (ten 26/25-bit limbs, the same bounds) and its fixed-base comb:
// base_comb() there is the k B of key generation and signing, on the twisted Edwards form -x^2 + y^2 = 1 + d x^2 y^2 that
// Ed25519 uses, from Ed25519's own base point.
//
//   scalars mod L      Barrett reduction in 32-bit words (HAC 14.42, b = 2^32, k = 8) and two masked subtractions: no branch
//   points             extended coordinates (X : Y : Z : T), x = X/Z, y = Y/Z, xy = T/Z; doubling and addition for a = -1
//                      (Hisil-Wong-Carter-Dawson 2008), additions against a cached form (Y+X, Y-X, 2dT, 2Z)
//   decoding           point.go:54-87: y < p, x = sqrt((y^2 - 1) / (d y^2 + 1)) by the (p-5)/8 power and sqrt(-1), x = 0 with
//                      the sign bit set rejected
//   verification       R' = [S]B + [k](-A) by one Horner pass over signed radix-16 digits of both scalars: 252 doublings,
//                      64 additions of a multiple of -A (eight multiples per lane in the caller's workspace) and 64 mixed
//                      additions of a multiple of B (row 0 of the comb).  Every input of verification is public: the
//                      multiples are read with per-lane addresses.
//
// Key generation and signing neither branch nor pick an address on the seed, s, the prefix, r or S: SHA-512 of a secret is
// straight-line code, the comb selects with wave-uniform addresses and compares, and the scalar arithmetic is masked.
#pragma once
#include <stdint.h>

#include "sha512_dev.h"
#include "x25519_dev.h"

namespace circl {
namespace ed25519 {

using x25519::Fe;
using x25519::fe_add;
using x25519::fe_const;
using x25519::fe_mul;
using x25519::fe_sqr;
using x25519::fe_sqr_n;
using x25519::fe_sub;

// ---- scalars modulo L = 2^252 + 27742317777372353535851937790883648493 (eight little-endian words) ----------------------
CIRCL_HD uint32_t order_word(int i) {
    constexpr uint32_t L[9] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u, 0u};
    return L[i];
}

// r = x - L if x >= L, else x (nine words; x < 2^288)
CIRCL_HD void sc_sub_order_if_ge(uint32_t x[9]) {
    uint32_t d[9], borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint64_t t = (uint64_t)x[i] - order_word(i) - borrow;
        d[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    const uint32_t keep = 0u - borrow;  // all ones iff x < L
#pragma unroll
    for (int i = 0; i < 9; i++) x[i] = (x[i] & keep) | (d[i] & ~keep);
}

// out = x mod L for a 512-bit x (sixteen little-endian words): ed25519.go reduceModOrder of a SHA-512 digest
CIRCL_HD void sc_reduce(uint32_t out[8], const uint32_t x[16]) {
    constexpr uint32_t MU[9] = {0x0a2c131bu, 0xed9ce5a3u, 0x086329a7u, 0x2106215du, 0xffffffebu,
                                0xffffffffu, 0xffffffffu, 0xffffffffu, 0x0000000fu};  // floor(2^512 / L)
    // q3 = floor(floor(x / 2^224) mu / 2^288): words 9..17 of the product of x[7..15] and mu
    uint32_t q2[18];
#pragma unroll
    for (int i = 0; i < 18; i++) q2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const uint64_t t = (uint64_t)x[7 + i] * MU[j] + q2[i + j] + c;
            q2[i + j] = (uint32_t)t;
            c = (uint32_t)(t >> 32);
        }
        q2[i + 9] = c;
    }
    // r = (x - q3 L) mod 2^288, below 3 L
    uint32_t r2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) r2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; i + j < 9; j++) {
            const uint64_t t = (uint64_t)q2[9 + i] * order_word(j) + r2[i + j] + c;
            r2[i + j] = (uint32_t)t;
            c = (uint32_t)(t >> 32);
        }
    }
    uint32_t r[9], borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint64_t t = (uint64_t)x[i] - r2[i] - borrow;
        r[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    sc_sub_order_if_ge(r);
    sc_sub_order_if_ge(r);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = r[i];
}

// out = (a b + c) mod L, a, b, c below 2^256: S = r + k s (ed25519.go calculateS)
CIRCL_HD void sc_muladd(uint32_t out[8], const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) {
    uint32_t p[16];
#pragma unroll
    for (int i = 0; i < 16; i++) p[i] = i < 8 ? c[i] : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t cy = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t t = (uint64_t)a[i] * b[j] + p[i + j] + cy;
            p[i + j] = (uint32_t)t;
            cy = (uint32_t)(t >> 32);
        }
        p[i + 8] = cy;  // rows before this one end at word i + 7
    }
    sc_reduce(out, p);
}

// 1 iff s < L (ed25519.go isLessThanOrder)
CIRCL_HD uint32_t sc_is_canonical(const uint32_t s[8]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)s[i] - order_word(i) - borrow;
        borrow = (uint32_t)(t >> 63);
    }
    return borrow;
}

// clamp(h[0..32)) of ed25519.go:392-396 on the first eight words of a digest
CIRCL_HD void clamp(uint32_t s[8]) {
    s[0] &= ~7u;
    s[7] = (s[7] & 0x7fffffffu) | 0x40000000u;
}

// ---- field helpers ----------------------------------------------------------------------------------------------------
CIRCL_HD Fe fe_lit(const uint32_t (&l)[10]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = l[i];
    return r;
}
CIRCL_HD Fe fe_d() {  // d = -121665 / 121666
    constexpr uint32_t l[10] = {0x35978a3u, 0xd37284u, 0x3156ebdu, 0x6a0a0eu, 0x1c029u, 0x179e898u, 0x3a03cbbu, 0x1ce7198u, 0x2e2b6ffu, 0x1480db3u};
    return fe_lit(l);
}
CIRCL_HD Fe fe_d2() {  // 2 d
    constexpr uint32_t l[10] = {0x2b2f159u, 0x1a6e509u, 0x22add7au, 0xd4141du, 0x38052u, 0xf3d130u, 0x3407977u, 0x19ce331u, 0x1c56dffu, 0x901b67u};
    return fe_lit(l);
}
CIRCL_HD Fe fe_sqrtm1() {  // 2^((p-1)/4), a square root of -1
    constexpr uint32_t l[10] = {0x20ea0b0u, 0x186c9d2u, 0x8f189du, 0x35697fu, 0xbd0c60u, 0x1fbd7a7u, 0x2804c9eu, 0x1e16569u, 0x4fc1du, 0xae0c92u};
    return fe_lit(l);
}

// one carry chain over a value with limbs below 2^32: the result is "carried" in the sense of x25519_dev.h
CIRCL_HD Fe fe_carry(const Fe &a) {
    uint64_t h[10];
#pragma unroll
    for (int i = 0; i < 10; i++) h[i] = a.v[i];
    return x25519::fe_carry64(h);
}
CIRCL_HD Fe fe_neg(const Fe &a) { return fe_sub(fe_const(0), a); }  // a carried; the result is below 2^27.1
CIRCL_HD Fe fe_select(const Fe &a, const Fe &b, bool take_b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = take_b ? b.v[i] : a.v[i];
    return r;
}

// z^((p-5)/8) = z^(2^252 - 3): the chain of fe_inv up to z^(2^250 - 1), then two squarings and a product by z
CIRCL_HD Fe fe_pow22523(const Fe &z) {
    const Fe z2 = fe_sqr(z);
    const Fe z9 = fe_mul(fe_sqr_n(z2, 2), z);
    const Fe z11 = fe_mul(z9, z2);
    const Fe z2_5_0 = fe_mul(fe_sqr(z11), z9);
    const Fe z2_10_0 = fe_mul(fe_sqr_n(z2_5_0, 5), z2_5_0);
    const Fe z2_20_0 = fe_mul(fe_sqr_n(z2_10_0, 10), z2_10_0);
    const Fe z2_40_0 = fe_mul(fe_sqr_n(z2_20_0, 20), z2_20_0);
    const Fe z2_50_0 = fe_mul(fe_sqr_n(z2_40_0, 10), z2_10_0);
    const Fe z2_100_0 = fe_mul(fe_sqr_n(z2_50_0, 50), z2_50_0);
    const Fe z2_200_0 = fe_mul(fe_sqr_n(z2_100_0, 100), z2_100_0);
    const Fe z2_250_0 = fe_mul(fe_sqr_n(z2_200_0, 50), z2_50_0);
    return fe_mul(fe_sqr_n(z2_250_0, 2), z);
}

CIRCL_HD bool words_equal(const uint32_t a[8], const uint32_t b[8]) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
    return d == 0;
}

// ---- points ---------------------------------------------------------------------------------------------------------
struct Ge {
    Fe X, Y, Z, T;
};
struct GeCached {  // (Y + X, Y - X, 2 d T, 2 Z)
    Fe YpX, YmX, T2d, Z2;
};

CIRCL_HD Ge ge_identity() { return {fe_const(0), fe_const(1), fe_const(1), fe_const(0)}; }
CIRCL_HD GeCached ge_cached_identity() { return {fe_const(1), fe_const(1), fe_const(0), fe_const(2)}; }

CIRCL_HD GeCached ge_to_cached(const Ge &p) { return {fe_add(p.Y, p.X), fe_sub(p.Y, p.X), fe_mul(p.T, fe_d2()), fe_add(p.Z, p.Z)}; }

// 2P (point.go double, a = -1): A = X^2, B = Y^2, C = 2 Z^2, H = A + B, E = (X + Y)^2 - H, G = B - A, F = C - G;
// (E F, G H, F G, E H).  H is carried before it is subtracted, F before it is multiplied.
CIRCL_HD Ge ge_dbl(const Ge &p) {
    const Fe A = fe_sqr(p.X), B = fe_sqr(p.Y);
    const Fe C = x25519::fe_mul_small(fe_sqr(p.Z), 2);
    const Fe H = fe_carry(fe_add(A, B));
    const Fe E = fe_sub(fe_sqr(fe_add(p.X, p.Y)), H);
    const Fe G = fe_sub(B, A);
    const Fe F = fe_carry(fe_sub(fe_add(C, A), B));  // C - G = C + A - B, carried: C + A + 2p would exceed the product bound
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

// P + Q, or P - Q when neg: A = (Y-X)(Y2-X2), B = (Y+X)(Y2+X2), C = T 2dT2, D = Z 2Z2; E = B - A, F = D - C, G = D + C,
// H = B + A; (E F, G H, F G, E H).  -Q swaps Y2+X2 with Y2-X2 and negates 2dT2, i.e. swaps F and G.
CIRCL_HD Ge ge_add(const Ge &p, const GeCached &q, bool neg) {
    const Fe A = fe_mul(fe_sub(p.Y, p.X), neg ? q.YpX : q.YmX);
    const Fe B = fe_mul(fe_add(p.Y, p.X), neg ? q.YmX : q.YpX);
    const Fe C = fe_mul(p.T, q.T2d), D = fe_mul(p.Z, q.Z2);
    const Fe E = fe_sub(B, A), H = fe_add(B, A);
    Fe F = fe_sub(D, C), G = fe_add(D, C);
    x25519::fe_cswap(F, G, neg ? 1u : 0u);
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

// P + Q for Q = ((y+x)/2, (y-x)/2, dxy) of the comb table (x25519_dev.h base_comb), or P - Q when neg
CIRCL_HD Ge ge_madd_half(const Ge &p, Fe q0, Fe q1, const Fe &q2, bool neg) {
    x25519::fe_cswap(q0, q1, neg ? 1u : 0u);
    const Fe A = fe_mul(fe_add(p.Y, p.X), q0), B = fe_mul(fe_sub(p.Y, p.X), q1), C = fe_mul(p.T, q2);
    const Fe E = fe_sub(A, B), H = fe_add(A, B);
    Fe G = fe_add(p.Z, C), F = fe_sub(p.Z, C);
    x25519::fe_cswap(G, F, neg ? 1u : 0u);
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}

// k B for k below 2^255 (the comb of x25519_dev.h)
CIRCL_HD Ge ge_base(const uint32_t k[8]) {
    const x25519::EdPoint p = x25519::base_comb(k);
    return {p.X, p.Y, p.Z, p.T};
}

// point.go ToBytes: y with the parity of x in bit 255 (eight little-endian words)
CIRCL_HD void ge_encode(uint32_t out[8], const Ge &p) {
    const Fe zi = x25519::fe_inv(p.Z);
    uint32_t xw[8];
    x25519::fe_to_words(xw, fe_mul(p.X, zi));
    x25519::fe_to_words(out, fe_mul(p.Y, zi));
    out[7] |= (xw[0] & 1u) << 31;
}

// point.go FromBytes (:54-87): 1 and the point (every coordinate carried), or 0 for an encoding the reference rejects
CIRCL_HD uint32_t ge_decode(Ge &p, const uint32_t in[8]) {
    const uint32_t sign = in[7] >> 31;
    uint32_t yw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) yw[i] = in[i];
    yw[7] &= 0x7fffffffu;
    bool ge_p = yw[7] == 0x7fffffffu && yw[0] >= 0xffffffedu;  // y >= p = 2^255 - 19
#pragma unroll
    for (int i = 1; i < 7; i++) ge_p = ge_p && yw[i] == 0xffffffffu;
    const Fe y = x25519::fe_from_words(yw);
    const Fe yy = fe_sqr(y);
    const Fe u = fe_carry(fe_sub(yy, fe_const(1)));          // y^2 - 1
    const Fe v = fe_carry(fe_add(fe_mul(yy, fe_d()), fe_const(1)));  // d y^2 + 1
    // x = u v^3 (u v^7)^((p-5)/8): a square root of u / v, or of -u / v
    const Fe v3 = fe_mul(fe_sqr(v), v);
    const Fe uv7 = fe_mul(u, fe_mul(fe_sqr(v3), v));
    Fe x = fe_mul(fe_mul(u, v3), fe_pow22523(uv7));
    uint32_t vxx[8], uw[8], nuw[8];
    x25519::fe_to_words(vxx, fe_mul(v, fe_sqr(x)));
    x25519::fe_to_words(uw, u);
    x25519::fe_to_words(nuw, fe_carry(fe_neg(u)));
    const bool root = words_equal(vxx, uw), flip = words_equal(vxx, nuw);
    x = fe_select(x, fe_mul(x, fe_sqrtm1()), !root);
    uint32_t xw[8];
    x25519::fe_to_words(xw, x);
    uint32_t xor_ = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) xor_ |= xw[i];
    const bool x_zero = xor_ == 0;
    x = fe_carry(fe_select(x, fe_neg(x), (xw[0] & 1u) != sign));
    p.X = x;
    p.Y = y;
    p.Z = fe_const(1);
    p.T = fe_mul(x, y);
    return (!ge_p && (root || flip) && !(x_zero && sign)) ? 1u : 0u;
}

// ---- verification: [s]B + [k]Q ------------------------------------------------------------------------------------------
// Signed radix-16 digits e_0..e_63 in [-8, 8] of a scalar below 2^253, produced top-down: with K = k + 0x0888..88 (8 added to
// nibbles 0..62), e_j = nibble_j(K) - 8 for j < 63 and e_63 = nibble_63(K) -- the same digits as the comb's bottom-up recoding.
CIRCL_HD void recode_prepare(uint32_t K[8], const uint32_t k[8]) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)k[i] + (i == 7 ? 0x08888888u : 0x88888888u) + c;
        K[i] = (uint32_t)t;
        c = (uint32_t)(t >> 32);
    }
}
// the next digit, top-down (K shifts left by one nibble)
CIRCL_HD int32_t recode_next(uint32_t K[8], bool top) {
    const int32_t e = (int32_t)(K[7] >> 28) - (top ? 0 : 8);
#pragma unroll
    for (int i = 7; i > 0; i--) K[i] = (K[i] << 4) | (K[i - 1] >> 28);
    K[0] <<= 4;
    return e;
}

// The eight multiples m Q (m = 1..8) in cached form, word-major across items: word w (0..39) of multiple m of item i sits at
// tab[((m - 1) 40 + w) stride + i], so that lanes reading the same multiple read consecutive words.
CIRCL_HD void table_store(uint32_t *tab, size_t stride, size_t i, int m, const GeCached &c) {
    uint32_t *t = tab + (size_t)(m - 1) * 40 * stride + i;
#pragma unroll
    for (int w = 0; w < 10; w++) {
        t[(size_t)w * stride] = c.YpX.v[w];
        t[(size_t)(10 + w) * stride] = c.YmX.v[w];
        t[(size_t)(20 + w) * stride] = c.T2d.v[w];
        t[(size_t)(30 + w) * stride] = c.Z2.v[w];
    }
}
CIRCL_HD GeCached table_load(const uint32_t *tab, size_t stride, size_t i, uint32_t m) {  // m in 0..8; 0 is the identity
    const uint32_t *t = tab + (size_t)(m ? m - 1 : 0) * 40 * stride + i;
    GeCached c;
#pragma unroll
    for (int w = 0; w < 10; w++) {
        c.YpX.v[w] = t[(size_t)w * stride];
        c.YmX.v[w] = t[(size_t)(10 + w) * stride];
        c.T2d.v[w] = t[(size_t)(20 + w) * stride];
        c.Z2.v[w] = t[(size_t)(30 + w) * stride];
    }
    return m ? c : ge_cached_identity();
}
CIRCL_HD void table_build(uint32_t *tab, size_t stride, size_t i, const Ge &q) {
    const GeCached c1 = ge_to_cached(q);
    table_store(tab, stride, i, 1, c1);
    Ge p = q;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int m = 2; m <= 8; m++) {
        p = ge_add(p, c1, false);
        table_store(tab, stride, i, m, ge_to_cached(p));
    }
}

// R = [s]B + [k]Q, s and k below 2^253 and PUBLIC (both digits pick addresses); Q's multiples from table_build
CIRCL_HD Ge double_scalar_mult(const uint32_t s[8], const uint32_t k[8], const uint32_t *tab, size_t stride, size_t i) {
    uint32_t S[8], K[8];
    recode_prepare(S, s);
    recode_prepare(K, k);
    Ge r = ge_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int j = 63; j >= 0; j--) {
        if (j != 63) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int d = 0; d < 4; d++) r = ge_dbl(r);
        }
        const int32_t ek = recode_next(K, j == 63), es = recode_next(S, j == 63);
        const uint32_t mk = (uint32_t)(ek < 0 ? -ek : ek), ms = (uint32_t)(es < 0 ? -es : es);
        r = ge_add(r, table_load(tab, stride, i, mk), ek < 0);
        // the comb's row 0 holds m B for m = 1..8; m = 0 is the identity ((1/2, 1/2, 0) in that form)
        const uint32_t *t = x25519::base_comb_entry(0, ms ? (int)ms - 1 : 0);
        Fe q0, q1, q2;
#pragma unroll
        for (int w = 0; w < 10; w++) {
            const uint32_t half = (w == 0) ? (x25519::M26 - 8) : (w == 9) ? 0xffffffu : x25519::limb_mask(w);
            q0.v[w] = ms ? t[w] : half;
            q1.v[w] = ms ? t[10 + w] : half;
            q2.v[w] = ms ? t[20 + w] : 0u;
        }
        r = ge_madd_half(r, q0, q1, q2, es < 0);
    }
    return r;
}

}  // namespace ed25519
}  // namespace circl
