// fp64_dev.h -- the field of Prio3Count / Prio3Sum: GF(p), p = 2^64 - 2^32 + 1 ("Goldilocks"; the reference's vdaf/prio3/arith/fp64),
// one element per lane.  An element is its canonical representative (< p) in a uint64_t at every load, store, argument and result:
// the reference's Montgomery form is internal to it, only the 8 little-endian canonical bytes are ever visible.
//
// The reduction uses 2^64 = 2^32 - 1 and 2^96 = -1 (mod p): a 128-bit product (lo, hi) is lo - hi[63:32] + hi[31:0] (2^32 - 1), a
// subtraction, one 32 x 32 -> 64 product and an addition, each with its wrap folded back by +- (2^32 - 1).  Nothing here branches on a
// value: the wraps and the final conditional subtraction are masks.  __host__ __device__, so tests/hostsim runs the same source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keccak_dev.h"

namespace circl {
namespace fp64 {

constexpr uint64_t P = 0xffffffff00000001ull;
constexpr uint64_t EPS = 0xffffffffull;   // 2^64 mod p

// all ones if c, else zero
CIRCL_HD uint64_t mask(bool c) { return (uint64_t)0 - (uint64_t)c; }
CIRCL_HD bool canonical(uint64_t x) { return x < P; }
// x < 2^64 to its canonical representative
CIRCL_HD uint64_t canon(uint64_t x) { return x - (P & mask(x >= P)); }

CIRCL_HD uint64_t add(uint64_t a, uint64_t b) {
    uint64_t s = a + b;
    s += EPS & mask(s < a);   // a + b < 2p: after a wrap s + EPS < p
    return canon(s);
}
CIRCL_HD uint64_t sub(uint64_t a, uint64_t b) {
    const uint64_t d = a - b;
    return d - (EPS & mask(a < b));   // a - b + p
}

CIRCL_HD uint64_t mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (hi 2^64 + lo) mod p
CIRCL_HD uint64_t reduce128(uint64_t lo, uint64_t hi) {
    const uint64_t hh = hi >> 32, hl = hi & EPS;
    uint64_t t0 = lo - hh;
    t0 -= EPS & mask(lo < hh);            // + p (mod 2^64)
    const uint64_t t1 = hl * EPS;         // < 2^64
    uint64_t r = t0 + t1;
    r += EPS & mask(r < t1);              // - p (mod 2^64); cannot wrap again: r < 2^64 - 2^32 before it
    return canon(r);
}
CIRCL_HD uint64_t mul(uint64_t a, uint64_t b) { return reduce128(a * b, mulhi(a, b)); }
CIRCL_HD uint64_t sqr(uint64_t a) { return mul(a, a); }

// a^e, e public
CIRCL_HD uint64_t pow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1) {
        if (e & 1) r = mul(r, a);
        a = sqr(a);
    }
    return r;
}
CIRCL_HD uint64_t inv(uint64_t a) { return pow(a, P - 2); }

// the root of unity of order 2^l, 7^((p - 1) / 2^l), l <= 8 (Prio3Sum's largest transform: 2P = 256 points)
CIRCL_HD uint64_t root_of_unity(int l) {
    constexpr uint64_t t[9] = {0x0000000000000001ull, 0xffffffff00000000ull, 0x0001000000000000ull, 0xfffffffeff000001ull,
                               0xefffffff00000001ull, 0x00003fffffffc000ull, 0x0000008000000000ull, 0xf80007ff08000001ull,
                               0xbf79143ce60ca966ull};
    return t[l];
}
// 2^-l: 2 has order 192 (2^96 = -1), so 2^-l = 2^(192 - l)
CIRCL_HD uint64_t inv_two_pow(int l) { return pow(2, 192 - l); }

}  // namespace fp64
}  // namespace circl
