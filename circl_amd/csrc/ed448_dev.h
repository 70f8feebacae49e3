// ed448_dev.h -- Ed448 (RFC 8032 5.2, pure, with context) on gfx950, one key / signature per lane.
//
// Replaces sign/ed448 (ed448.go) and what it uses of ecc/goldilocks (point.go, scalar.go, curve.go, twist*.go, isogeny.go) for
// batch key generation, signing and verification, on the GF(2^448 - 2^224 - 1) arithmetic of fp448_dev.h.  The reference
// computes on a 4-isogenous twisted curve; this file stays on the Edwards curve x^2 + y^2 = 1 + d x^2 y^2, d = -39081, and
// reproduces the reference's bytes and verdicts.
//
//   scalars mod l      l = 2^446 - c with c below 2^224: a 912-bit SHAKE256 output is folded three times (x = hi 2^446 + lo
//                      becomes hi c + lo) and one masked subtraction finishes it: no branch
//   points             extended coordinates (X : Y : Z : T), a = 1; unified addition (Hisil-Wong-Carter-Dawson 2008, 9 products)
//                      and doubling (4 squarings + 4 products, 3 when the next operation is another doubling); both complete
//   decoding           ecc/goldilocks point.go:43-80: the low seven bits of byte 56 zero, y < p, x = sqrt((1 - y^2) / (39081 y^2 + 1))
//                      exists, x = 0 with the sign bit set rejected
//   fixed base         k B by 112 signed radix-16 digits in eight blocks of fourteen over the eight rows of ed448_base_table.h:
//                      thirteen runs of four doublings and 112 mixed additions.  The candidates of a digit are the same for every
//                      lane: they are read with wave-uniform addresses and selected by compares, so neither addresses nor control
//                      flow depend on the scalar.
//   verification       the reference's rule, which is neither cofactorless nor RFC 8032's cofactored one: goldilocks.Curve.
//                      CombinedMult (curve.go:80-90) divides both scalars by 4 mod l, works on the isogenous curve and comes
//                      back, which multiplies by 4.  Here: Q' = [S/4 mod l]B + [k/4 mod l](-A) by one Horner pass over signed
//                      radix-16 digits of both scalars (444 doublings, 112 additions of a multiple of -A from the caller's
//                      workspace, 112 mixed additions of a multiple of B), Q = 4 Q', and enc(Q) is compared with the 57 bytes
//                      of R.  A's 4-torsion component drops out; one in R does not.  Every input is public: the multiples are
//                      read with per-lane addresses.
//   SHAKE256           dom4 || context || a register-held part || message, 136 bytes per block; the context and the message come
//                      straight from the ragged blobs at any byte alignment, the register-held part is placed at its byte
//                      offset by compares (it may be secret: the prefix), 114 bytes out of one squeeze block
//
// Key generation and signing neither branch nor pick an address on the seed, s, the prefix, r or S.
#pragma once
#include <stdint.h>

#include "keccak_dev.h"
#include "fp448_dev.h"
#include "ed448_base_table.h"

namespace circl {
namespace ed448 {

using fp448::Fe;
using fp448::fe_add;
using fp448::fe_const;
using fp448::fe_mul;
using fp448::fe_mul_small;
using fp448::fe_neg;
using fp448::fe_select;
using fp448::fe_sqr;
using fp448::fe_sub;

// ---- scalars modulo l = 2^446 - c (fourteen little-endian words) ---------------------------------------------------------
CIRCL_HD uint32_t order_word(int i) {
    constexpr uint32_t L[14] = {0xab5844f3u, 0x2378c292u, 0x8dc58f55u, 0x216cc272u, 0xaed63690u, 0xc44edb49u, 0x7cca23e9u,
                                0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
    return L[i];
}
CIRCL_HD uint32_t order_c_word(int i) {  // c = 2^446 - l, 224 bits
    constexpr uint32_t Cw[7] = {0x54a7bb0du, 0xdc873d6du, 0x723a70aau, 0xde933d8du, 0x5129c96fu, 0x3bb124b6u, 0x8335dc16u};
    return Cw[i];
}

// y = (x mod 2^446) + floor(x / 2^446) c for an x of NX words; y has NY = max(NX - 6, 15) words
template <int NX>
struct Fold {
    static constexpr int NH = NX - 13, NY = NX - 6 > 15 ? NX - 6 : 15;
};
template <int NX>
CIRCL_HD void sc_fold(uint32_t *y, const uint32_t *x) {
    constexpr int NH = Fold<NX>::NH, NY = Fold<NX>::NY;
#pragma unroll
    for (int i = 0; i < NY; i++) y[i] = i < 13 ? x[i] : (i == 13 ? x[13] & 0x3fffffffu : 0u);
#pragma unroll
    for (int i = 0; i < NH; i++) {
        const uint32_t h = (x[13 + i] >> 30) | (13 + i + 1 < NX ? x[14 + i] << 2 : 0u);
        uint32_t cy = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const uint64_t t = (uint64_t)h * order_c_word(j) + y[i + j] + cy;
            y[i + j] = (uint32_t)t;
            cy = (uint32_t)(t >> 32);
        }
#pragma unroll
        for (int j = i + 7; j < NY; j++) {  // the carry runs on (the sum fits NY words)
            const uint64_t t = (uint64_t)y[j] + cy;
            y[j] = (uint32_t)t;
            cy = (uint32_t)(t >> 32);
        }
    }
}

// x - l if x >= l, else x (fourteen words)
CIRCL_HD void sc_sub_order_if_ge(uint32_t x[14]) {
    uint32_t d[14], borrow = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint64_t t = (uint64_t)x[i] - order_word(i) - borrow;
        d[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    const uint32_t keep = 0u - borrow;  // all ones iff x < l
#pragma unroll
    for (int i = 0; i < 14; i++) x[i] = (x[i] & keep) | (d[i] & ~keep);
}

// out = x mod l for a 912-bit x (29 words, the top one 16 bits): the reduction of a 114-byte SHAKE256 output
CIRCL_HD void sc_reduce(uint32_t out[14], const uint32_t x[29]) {
    uint32_t y1[Fold<29>::NY], y2[Fold<23>::NY], y3[Fold<17>::NY];
    static_assert(Fold<29>::NY == 23 && Fold<23>::NY == 17 && Fold<17>::NY == 15, "fold sizes");
    sc_fold<29>(y1, x);   // below 2^691
    sc_fold<23>(y2, y1);  // below 2^469
    sc_fold<17>(y3, y2);  // below 2^446 + 2^247
    sc_sub_order_if_ge(y3);
#pragma unroll
    for (int i = 0; i < 14; i++) out[i] = y3[i];
}

// out = x mod l for x below 2^448 (the clamped secret scalar: [s]B = [s mod l]B, and the fixed-base routine wants k < 2^446)
CIRCL_HD void sc_reduce_small(uint32_t out[14], const uint32_t x[14]) {
    uint32_t t[17], y[15];
#pragma unroll
    for (int i = 0; i < 17; i++) t[i] = i < 14 ? x[i] : 0u;
    sc_fold<17>(y, t);
    sc_sub_order_if_ge(y);
#pragma unroll
    for (int i = 0; i < 14; i++) out[i] = y[i];
}

// out = (a b + c) mod l, a, b, c below 2^448: S = r + k s
CIRCL_HD void sc_muladd(uint32_t out[14], const uint32_t a[14], const uint32_t b[14], const uint32_t c[14]) {
    uint32_t p[29];
#pragma unroll
    for (int i = 0; i < 29; i++) p[i] = i < 14 ? c[i] : 0u;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        uint32_t cy = 0;
#pragma unroll
        for (int j = 0; j < 14; j++) {
            const uint64_t t = (uint64_t)a[i] * b[j] + p[i + j] + cy;
            p[i + j] = (uint32_t)t;
            cy = (uint32_t)(t >> 32);
        }
        p[i + 14] += cy;  // rows before this one end at word i + 13 (plus c's carry, which fits)
    }
    sc_reduce(out, p);
}

// 1 iff the 57-byte S (fourteen words and byte 56) is below l: ed448.go isLessThanOrder compares all 57 bytes, so byte 56 must be 0
CIRCL_HD uint32_t sc_is_canonical(const uint32_t s[15]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint64_t t = (uint64_t)s[i] - order_word(i) - borrow;
        borrow = (uint32_t)(t >> 63);
    }
    return borrow & ((s[14] & 0xffu) == 0 ? 1u : 0u);
}

// x / 4 mod l for x below l: l = 3 mod 4, so x + (x mod 4) l is divisible by 4 (and below 2^448)
CIRCL_HD void sc_div4(uint32_t out[14], const uint32_t x[14]) {
    const uint32_t m = x[0] & 3u;
    uint32_t t[14], cy = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint64_t v = (uint64_t)m * order_word(i) + x[i] + cy;
        t[i] = (uint32_t)v;
        cy = (uint32_t)(v >> 32);
    }
#pragma unroll
    for (int i = 0; i < 14; i++) out[i] = (t[i] >> 2) | (i < 13 ? t[i + 1] << 30 : 0u);
}

// deriveSecretScalar (ed448.go): h[0] &= 0xFC, h[55] |= 0x80, h[56] = 0, on the first fourteen words of SHAKE256(seed, 114)
CIRCL_HD void clamp(uint32_t s[14]) {
    s[0] &= ~3u;
    s[13] |= 0x80000000u;
}

// ---- bytes at any alignment ------------------------------------------------------------------------------------------------
// The little-endian word of bytes ptr[q .. q + 4) with the bytes outside [0, len) zero; q may be negative or past the end.  The
// bytes are read as the one or two ALIGNED dwords that hold them (joined by V_ALIGNBIT_B32), and a dword is read only if it holds
// a byte of the row, so no read leaves the 4-byte-aligned words the row touches.
CIRCL_HD uint32_t bytes_word(const uint8_t *ptr, uint64_t len, int64_t q) {
    if (q <= -4 || q >= (int64_t)len) return 0u;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(ptr), hi = lo + len, a = lo + (uintptr_t)q, base = a & ~(uintptr_t)3;
    const uint32_t w0 = base + 4 > lo ? *reinterpret_cast<const uint32_t *>(base) : 0u;
    const uint32_t w1 = base + 4 < hi ? *reinterpret_cast<const uint32_t *>(base + 4) : 0u;
    uint32_t v = alignbit(w1, w0, (uint32_t)(a & 3) * 8);
    if (q < 0) v &= 0xffffffffu << (8 * (uint32_t)(-q));
    const int64_t rem = (int64_t)len - q;
    if (rem < 4) v &= (1u << (8 * (uint32_t)rem)) - 1u;
    return v;
}
template <int NW>
CIRCL_HD void load_row(uint32_t (&w)[NW], const uint8_t *ptr, uint32_t nbytes) {
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] = bytes_word(ptr, nbytes, 4 * k);
}
template <int NW>
CIRCL_HD void store_row(uint8_t *ptr, const uint32_t (&w)[NW], int nbytes) {
#pragma unroll
    for (int b = 0; b < 4 * NW; b++)
        if (b < nbytes) ptr[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}

// ---- SHAKE256(dom4(ctx) || mid || msg, 114) --------------------------------------------------------------------------------
// DOM: the stream opens with "SigEd448" || 0x00 || clen || ctx[0 .. clen) (clen <= 255); otherwise it starts at mid.
// mid: MW words of which the first mid_bytes bytes count (the bytes behind them must be zero); it may be secret, so it is placed
// by compares against every word index, never by an address.  out: the 114 bytes as 29 words (the top one 16 bits).
template <bool DOM, int MW>
CIRCL_HD void shake256_114(uint32_t out[29], const uint8_t *ctx, uint32_t clen, const uint32_t (&mid)[MW], uint32_t mid_bytes, const uint8_t *msg,
                           uint64_t mlen) {
    const int64_t o = DOM ? 10 + (int64_t)clen : 0;  // where mid starts
    const int64_t m0 = o + mid_bytes;                // where the message starts
    const int64_t total = m0 + (int64_t)mlen;
    const int64_t nblocks = total / 136 + 1;
    KeccakState st;
    keccak_zero(st);
    for (int64_t blk = 0; blk < nblocks; blk++) {
        const int64_t base = blk * 136;
        uint32_t g[35];
#pragma unroll
        for (int j = 0; j < 35; j++) g[j] = 0u;
        const int64_t rel = base - o;
        const uint32_t bs = (uint32_t)(rel & 3) * 8;
        if (base + 136 > o && base < m0) {  // (public: lengths only)
            const int32_t wi0 = (int32_t)(rel >> 2);
#pragma unroll
            for (int j = 0; j < 35; j++) {
                const int32_t k = wi0 + j;
                uint32_t v = 0u;
#pragma unroll
                for (int s = 0; s < MW; s++) v = (k == s) ? mid[s] : v;
                g[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 34; j++) {
            const int64_t p = base + 4 * j;
            uint32_t w = alignbit(g[j + 1], g[j], bs);
            if (DOM) {
                if (blk == 0 && j < 3) w |= j == 0 ? 0x45676953u : j == 1 ? 0x38343464u : (clen << 8);  // "SigE", "d448", 0x00 || clen
                w |= bytes_word(ctx, clen, p - 10);
            }
            w |= bytes_word(msg, mlen, p - m0);
            if (total >= p && total < p + 4) w ^= 0x1fu << (8 * (uint32_t)(total - p));
            if (j & 1) st.hi[j >> 1] ^= w;
            else st.lo[j >> 1] ^= w;
        }
        if (blk == nblocks - 1) st.hi[16] ^= 0x80000000u;
        keccak_f1600(st);
    }
#pragma unroll
    for (int j = 0; j < 14; j++) {
        out[2 * j] = st.lo[j];
        out[2 * j + 1] = st.hi[j];
    }
    out[28] = st.lo[14] & 0xffffu;
}

// ---- points ---------------------------------------------------------------------------------------------------------------
struct Ge {
    Fe X, Y, Z, T;
};
struct GeCached {  // (X, Y, Z, 39081 T), every coordinate carried
    Fe X, Y, Z, Td;
};

CIRCL_HD Ge ge_identity() { return {fe_const(0), fe_const(1), fe_const(1), fe_const(0)}; }
CIRCL_HD GeCached ge_to_cached(const Ge &p) { return {p.X, p.Y, p.Z, fe_mul_small(p.T, 39081)}; }

// 2P (a = 1): A = X^2, B = Y^2, C = 2 Z^2, G = A + B, E = (X + Y)^2 - A - B, F = G - C, H = A - B; (E F, G H, F G, E H).
// want_t (wave-uniform): T is needed only when an addition follows.
CIRCL_HD Ge ge_dbl(const Ge &p, bool want_t) {
    const Fe A = fe_sqr(p.X), B = fe_sqr(p.Y);
    const Fe C = fe_mul_small(fe_sqr(p.Z), 2);
    const Fe G = fe_add(A, B);
    const Fe E = fe_sub(fe_sub(fe_sqr(fe_add(p.X, p.Y)), A), B);
    const Fe F = fe_sub(G, C), H = fe_sub(A, B);
    Ge r;
    r.X = fe_mul(E, F);
    r.Y = fe_mul(G, H);
    r.Z = fe_mul(F, G);
    r.T = p.T;
    if (want_t) r.T = fe_mul(E, H);
    return r;
}

// P + (x2 : y2 : z2) with w = 39081 T1 t2 and dz = Z1 z2 given: A = X1 x2, B = Y1 y2, E = (X1 + Y1)(x2 + y2) - A - B,
// F = dz + w (d = -39081), G = dz - w, H = B - A; (E F, G H, F G, E H)
CIRCL_HD Ge ge_add_core(const Ge &p, const Fe &x2, const Fe &y2, const Fe &w, const Fe &dz) {
    const Fe A = fe_mul(p.X, x2), B = fe_mul(p.Y, y2);
    const Fe E = fe_sub(fe_sub(fe_mul(fe_add(p.X, p.Y), fe_add(x2, y2)), A), B);
    const Fe F = fe_add(dz, w), G = fe_sub(dz, w), H = fe_sub(B, A);
    return {fe_mul(E, F), fe_mul(G, H), fe_mul(F, G), fe_mul(E, H)};
}
// P + Q, or P - Q when neg (-Q negates X and T)
CIRCL_HD Ge ge_add(const Ge &p, const GeCached &q, bool neg) {
    const Fe x2 = fe_select(q.X, fe_neg(q.X), neg), td = fe_select(q.Td, fe_neg(q.Td), neg);
    return ge_add_core(p, x2, q.Y, fe_mul(p.T, td), fe_mul(p.Z, q.Z));
}
// P + Q for an affine Q = (x, y, 39081 x y) of the base table, or P - Q when neg
CIRCL_HD Ge ge_madd(const Ge &p, const Fe &x, const Fe &y, const Fe &td, bool neg) {
    const Fe x2 = fe_select(x, fe_neg(x), neg), t2 = fe_select(td, fe_neg(td), neg);
    return ge_add_core(p, x2, y, fe_mul(p.T, t2), p.Z);
}

// point.go ToBytes: y (fourteen words) and the parity of x in bit 7 of byte 56 (word 14)
CIRCL_HD void ge_encode(uint32_t out[15], const Ge &p) {
    const Fe zi = fp448::fe_inv(p.Z);
    uint32_t xw[14];
    fp448::fe_to_words(xw, fe_mul(p.X, zi));
    fp448::fe_to_words(out, fe_mul(p.Y, zi));
    out[14] = (xw[0] & 1u) << 7;
}

// point.go FromBytes (:43-80) on the 57 bytes as fifteen words: 1 and the point (every coordinate carried), or 0 for an
// encoding the reference rejects
CIRCL_HD uint32_t ge_decode(Ge &p, const uint32_t in[15]) {
    const uint32_t sign = (in[14] >> 7) & 1u;
    const bool low7 = (in[14] & 0x7fu) != 0;
    const Fe y = fp448::fe_from_words(in);
    uint32_t yw[14], dif = 0;
    fp448::fe_to_words(yw, y);
#pragma unroll
    for (int i = 0; i < 14; i++) dif |= yw[i] ^ in[i];  // y >= p iff its canonical value differs
    const Fe yy = fe_sqr(y);
    const Fe u = fe_sub(fe_const(1), yy);                        // 1 - y^2
    Fe v = fe_mul_small(yy, 39081);                              // 39081 y^2 + 1 = -(d y^2 - 1)
    v.v[0] += 1;
    Fe x;
    const bool square = fp448::fe_sqrt_ratio(x, u, v);
    uint32_t xw[14], xo = 0;
    fp448::fe_to_words(xw, x);
#pragma unroll
    for (int i = 0; i < 14; i++) xo |= xw[i];
    x = fe_select(x, fe_neg(x), (xw[0] & 1u) != sign);
    p.X = x;
    p.Y = y;
    p.Z = fe_const(1);
    p.T = fe_mul(x, y);
    return (!low7 && dif == 0 && square && !(xo == 0 && sign)) ? 1u : 0u;
}

// ---- fixed base ------------------------------------------------------------------------------------------------------------
// the table entry selected by m in 0..8 (0: the identity (0, 1, 0)) from row b, by compares over wave-uniform reads
CIRCL_HD void base_select(Fe &x, Fe &y, Fe &td, int b, uint32_t m) {
    x = fe_const(0);
    y = fe_const(1);
    td = fe_const(0);
#pragma unroll
    for (int mm = 0; mm < 8; mm++) {
        const uint32_t *t = base_table_entry(b, mm);
        const uint32_t mask = 0u - (((m ^ (uint32_t)(mm + 1)) - 1u) >> 31);  // all ones iff m == mm + 1; no branch
#pragma unroll
        for (int i = 0; i < 16; i++) {
            x.v[i] ^= mask & (x.v[i] ^ t[i]);
            y.v[i] ^= mask & (y.v[i] ^ t[16 + i]);
            td.v[i] ^= mask & (td.v[i] ^ t[32 + i]);
        }
    }
}

// K = k + 0x88...8 for k below 2^446: the signed radix-16 digit j of k is nibble_j(K) - 8, in [-8, 7]
CIRCL_HD void recode_prepare(uint32_t K[14], const uint32_t k[14]) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const uint64_t t = (uint64_t)k[i] + 0x88888888u + c;
        K[i] = (uint32_t)t;
        c = (uint32_t)(t >> 32);
    }
}

// k B for k below 2^446 (+ a little: the top nibble must stay below 8).  With K = k + 0x88...8 the signed digit j is
// nibble_j(K) - 8, in [-8, 7].  Block b (digits 14 b .. 14 b + 13) sits in the top 56 bits of blk[b]; the block in turn is
// always blk[0] (the array rotates), so that no register is picked by an index.
CIRCL_HD Ge ge_base(const uint32_t k[14]) {
    uint32_t K[14];
    recode_prepare(K, k);
    uint64_t blk[8];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const int q = (56 * b) >> 5, r = (56 * b) & 31;
        const uint32_t w0 = K[q], w1 = K[q + 1], w2 = q + 2 < 14 ? K[q + 2] : 0u;
        const uint32_t lo = r ? (w0 >> r) | (w1 << (32 - r)) : w0, hi = r ? (w1 >> r) | (w2 << (32 - r)) : w1;
        blk[b] = (((uint64_t)hi << 32) | lo) << 8;
    }
    Ge p = ge_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 13; i >= 0; i--) {
        if (i != 13) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int d = 0; d < 4; d++) p = ge_dbl(p, d == 3);
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int b = 0; b < 8; b++) {
            const int32_t e = (int32_t)(blk[0] >> 60) - 8;
            const uint64_t first = blk[0] << 4;
#pragma unroll
            for (int j = 0; j < 7; j++) blk[j] = blk[j + 1];
            blk[7] = first;
            const bool neg = e < 0;
            Fe x, y, td;
            base_select(x, y, td, b, (uint32_t)(neg ? -e : e));
            p = ge_madd(p, x, y, td, neg);
        }
    }
    return p;
}

// ---- verification: [s]B + [k]Q ------------------------------------------------------------------------------------------------
// The eight multiples m Q (m = 1..8) in cached form, word-major across items: word w (0..63) of multiple m of item i sits at
// tab[((m - 1) 64 + w) stride + i], so that lanes reading the same multiple read consecutive words.
constexpr int kTableWords = 8 * 64;
CIRCL_HD void table_store(uint32_t *tab, size_t stride, size_t i, int m, const GeCached &c) {
    uint32_t *t = tab + (size_t)(m - 1) * 64 * stride + i;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        t[(size_t)w * stride] = c.X.v[w];
        t[(size_t)(16 + w) * stride] = c.Y.v[w];
        t[(size_t)(32 + w) * stride] = c.Z.v[w];
        t[(size_t)(48 + w) * stride] = c.Td.v[w];
    }
}
CIRCL_HD GeCached table_load(const uint32_t *tab, size_t stride, size_t i, uint32_t m) {  // m in 0..8; 0 is the identity
    const uint32_t *t = tab + (size_t)(m ? m - 1 : 0) * 64 * stride + i;
    GeCached c;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        c.X.v[w] = m ? t[(size_t)w * stride] : 0u;
        c.Y.v[w] = m ? t[(size_t)(16 + w) * stride] : (w == 0 ? 1u : 0u);
        c.Z.v[w] = m ? t[(size_t)(32 + w) * stride] : (w == 0 ? 1u : 0u);
        c.Td.v[w] = m ? t[(size_t)(48 + w) * stride] : 0u;
    }
    return c;
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

// [s]B + [k]Q for PUBLIC s and k below 2^446 (both digits pick addresses).  rec: the recoded scalars (recode_prepare), word w of
// S at rec[w stride + i] and word w of K at rec[(14 + w) stride + i]: the loop reads the one word that holds its digit (the word
// index is wave-uniform) instead of keeping 28 words alive.  tab: Q's multiples from table_build.
constexpr int kRecodedWords = 28;
CIRCL_HD Ge double_scalar_mult(const uint32_t *rec, const uint32_t *tab, size_t stride, size_t i) {
    Ge r = ge_identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int j = 111; j >= 0; j--) {
        if (j != 111) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int d = 0; d < 4; d++) r = ge_dbl(r, d == 3);
        }
        const uint32_t sh = 4u * (uint32_t)(j & 7);
        const int32_t es = (int32_t)((rec[(size_t)(j >> 3) * stride + i] >> sh) & 15u) - 8;
        const int32_t ek = (int32_t)((rec[(size_t)(14 + (j >> 3)) * stride + i] >> sh) & 15u) - 8;
        const uint32_t mk = (uint32_t)(ek < 0 ? -ek : ek), ms = (uint32_t)(es < 0 ? -es : es);
        r = ge_add(r, table_load(tab, stride, i, mk), ek < 0);
        const uint32_t *t = base_table_entry(0, ms ? (int)ms - 1 : 0);  // row 0 holds m B for m = 1..8
        Fe x, y, td;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            x.v[w] = ms ? t[w] : 0u;
            y.v[w] = ms ? t[16 + w] : (w == 0 ? 1u : 0u);
            td.v[w] = ms ? t[32 + w] : 0u;
        }
        r = ge_madd(r, x, y, td, es < 0);
    }
    return r;
}

// The recoded forms of s / 4 and k / 4 mod l (s, k below l) for combined_mult
CIRCL_HD void recode_store_div4(uint32_t *rec, size_t stride, size_t i, int which, const uint32_t x[14]) {
    uint32_t q[14], K[14];
    sc_div4(q, x);
    recode_prepare(K, q);
#pragma unroll
    for (int w = 0; w < 14; w++) rec[(size_t)(14 * which + w) * stride + i] = K[w];
}

// What goldilocks.Curve.CombinedMult(s, k, Q) returns: 4 ([s/4]B + [k/4]Q); rec from recode_store_div4 (0: s, 1: k), tab Q's multiples
CIRCL_HD Ge combined_mult(const uint32_t *rec, const uint32_t *tab, size_t stride, size_t i) {
    return ge_dbl(ge_dbl(double_scalar_mult(rec, tab, stride, i), false), false);
}

}  // namespace ed448
}  // namespace circl
