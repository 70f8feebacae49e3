// x448_dev.h -- X448 (RFC 7748) on gfx950, one scalar multiplication per lane.
//
// Replaces dh/x448 (key.go, curve.go, curve_generic.go, table.go and the ADX/BMI2 assembler) on the GF(2^448 - 2^224 - 1)
// arithmetic of fp448_dev.h.  The ladder is RFC 7748's (448 steps, a24 = 39081), which computes the same x/z as the
// reference's ladderMontgomery; conditional swaps are per-lane selects on the scalar bit.  Per step: A = x2 + z2 and
// C = x3 + z3 are sums of two carried values, B = x2 - z2 and D = x3 - z3 differences (as good as carried), every product
// has at most sums of two on both sides (fp448_dev.h's bound).
//
// KeyGen has two routes.  The ladder from u = 5 (the product by x1 becomes a product by the constant), and the fixed-base comb of
// Ed448 (base_mult_comb): RFC 7748's 4-isogeny (x, y) -> u = y^2 / x^2 from edwards448 to curve448 is a group homomorphism that
// sends the Ed448 base point B to the point with u = 5, so u([k]B) = X448(k, 5) for every k, with no factor to undo
// (tests/test_x448_comb_hostsim.py checks the identity on integers).  The reference uses a right-to-left Joye ladder over a
// table of multiples (ladderJoye, table.go).  Both routes give the reference's bytes.
#pragma once
#include <stdint.h>

#include "ed448_dev.h"
#include "fp448_dev.h"

namespace circl {
namespace x448 {

using fp448::Fe;
using fp448::fe_add;
using fp448::fe_const;
using fp448::fe_cswap;
using fp448::fe_mul;
using fp448::fe_mul_small;
using fp448::fe_sqr;
using fp448::fe_sub;

// key.go:22-30 isValidPubKey on the 56 point bytes as words: the value is reduced mod p and compared with lowOrderPoints
// (curve.go:76: 0, 1, p - 1), so the unreduced aliases p and p + 1 are low-order too.  Returns 1 for a valid key.
CIRCL_HD uint32_t valid_public(const uint32_t u[14]) {
    // p = 2^448 - 2^224 - 1: words 0..6 ffffffff, word 7 fffffffe, words 8..13 ffffffff
    uint32_t lo_or = 0, lo_and = 0xffffffffu, hi_or = 0, hi_and = 0xffffffffu;
#pragma unroll
    for (int i = 1; i < 7; i++) {
        lo_or |= u[i];
        lo_and &= u[i];
    }
#pragma unroll
    for (int i = 8; i < 14; i++) {
        hi_or |= u[i];
        hi_and &= u[i];
    }
    const bool small = (lo_or | hi_or | u[7]) == 0 && u[0] <= 1;                                                     // 0, 1
    const bool near_p = hi_and == 0xffffffffu && lo_and == 0xffffffffu && u[7] == 0xfffffffeu && u[0] >= 0xfffffffeu;  // p - 1, p
    const bool p_plus_1 = hi_and == 0xffffffffu && u[7] == 0xffffffffu && (lo_or | u[0]) == 0;                        // p + 1
    return (small || near_p || p_plus_1) ? 0u : 1u;
}

// X448(k, u): k = the 56 scalar bytes as words (clamped here, key.go:15-20), u = the 56 point bytes as words (any value below
// 2^448: the field arithmetic reduces it).  BASE: u = 5 (KeyGen, key.go:33-35).
template <bool BASE>
CIRCL_HD void scalar_mult(uint32_t out[14], const uint32_t k_in[14], const uint32_t u_in[14]) {
    uint32_t k[14];
#pragma unroll
    for (int i = 0; i < 14; i++) k[i] = k_in[i];
    k[0] &= ~3u;
    k[13] |= 0x80000000u;
    Fe x1 = fe_const(5);
    if (!BASE) x1 = fp448::fe_from_words(u_in);
    Fe x2 = fe_const(1), z2 = fe_const(0), x3 = x1, z3 = fe_const(1);
    uint32_t swap = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = 447; t >= 0; t--) {
        const uint32_t bit = k[13] >> 31;  // the current bit is always the top bit: the scalar shifts left
#pragma unroll
        for (int i = 13; i > 0; i--) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
        k[0] <<= 1;
        swap ^= bit;
        fe_cswap(x2, x3, swap);
        fe_cswap(z2, z3, swap);
        swap = bit;
        const Fe A = fe_add(x2, z2), B = fe_sub(x2, z2);
        const Fe C = fe_add(x3, z3), D = fe_sub(x3, z3);
        const Fe DA = fe_mul(D, A), CB = fe_mul(C, B);
        const Fe AA = fe_sqr(A), BB = fe_sqr(B);
        x3 = fe_sqr(fe_add(DA, CB));
        const Fe t1 = fe_sqr(fe_sub(DA, CB));
        z3 = BASE ? fe_mul_small(t1, 5) : fe_mul(x1, t1);
        x2 = fe_mul(AA, BB);
        const Fe E = fe_sub(AA, BB);
        z2 = fe_mul(E, fe_add(AA, fe_mul_small(E, 39081)));  // RFC 7748: E (AA + a24 E)
    }
    fe_cswap(x2, x3, swap);
    fe_cswap(z2, z3, swap);
    fp448::fe_to_words(out, fe_mul(x2, fp448::fe_inv(z2)));
}

// X448(k, 5) on the fixed-base comb of ed448_dev.h: 112 mixed additions and 52 doublings against 448 ladder steps.  k is clamped
// as in scalar_mult, then reduced mod l (ge_base wants k below 2^446; B has order l, so [k]B depends on k mod l only).  A clamped
// k is a multiple of 4 in [2^447, 2^448), which holds 3 l (not a multiple of 4) and 4 l: k = 4 l is the one clamped scalar with
// [k]B the identity (0, 1).  Then X = 0, fe_inv sends 0 to 0 and u = 0, which is what the ladder's x / z gives at the point at
// infinity.  Everywhere else X != 0 and u = Y^2 / X^2 (Z cancels).  No branch and no address depends on k (base_select).
CIRCL_HD void base_mult_comb(uint32_t out[14], const uint32_t k_in[14]) {
    uint32_t k[14], r[14];
#pragma unroll
    for (int i = 0; i < 14; i++) k[i] = k_in[i];
    ed448::clamp(k);
    ed448::sc_reduce_small(r, k);
    const ed448::Ge p = ed448::ge_base(r);
    fp448::fe_to_words(out, fe_mul(fe_sqr(p.Y), fp448::fe_inv(fe_sqr(p.X))));
}

}  // namespace x448
}  // namespace circl
