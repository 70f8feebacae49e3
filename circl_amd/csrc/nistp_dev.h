// nistp_dev.h -- the NIST P-256 and P-384 prime-order groups on gfx950, one element per lane, with hash-to-curve and hash-to-scalar
// (RFC 9380: expand_message_xmd over SHA-256 / SHA-384, hash_to_field, simplified SWU for p = 3 mod 4).
//
// Replaces group/short.go (which hands the arithmetic to big integers and crypto/elliptic) for batch work.  One template over a curve
// description (struct P256, struct P384: limb count, p, b, the order n, the Montgomery constants of both moduli, the SSWU constants Z
// and c2, L, the hash), written from SEC 1, FIPS 186-4 D.1.2, RFC 9380 and eprint 2015/1060.  No LDS, no workspace.
//
//   Fe<N>             N limbs of 32 bits, little-endian, ALWAYS fully reduced (below the modulus), so that equality, zero and sign tests are
//                     on canonical words.  Field elements are in Montgomery form (x R, R = 2^(32 N)); scalars are plain integers.
//   mont_mul          coarsely integrated operand scanning, 32 x 32 -> 64 multiply-adds, one conditional subtraction.  Both primes are
//                     -1 mod 2^32, so -p^-1 mod 2^32 = 1 and the factor of a row is the row's low limb itself (Mod::NINV = 1 folds
//                     away); the orders carry a real constant.
//   fe_pow_c1         x^((p - 3) / 4), square-and-multiply over the PUBLIC exponent p >> 2 (its bits steer wave-uniform branches).  The
//                     square root x^((p + 1) / 4) = x x^c1, the inverse x^(p - 2) = (x^c1)^4 x and the SSWU power are all this one power.
//   sc_mul / sc_inv   products mod n; x^(n - 2) over the public exponent.  0 maps to 0: the caller masks it.
//   reduce_wide       an L-byte big-endian string (L = 48 / 72) modulo p or n: lo R + hi R^2 through two Montgomery products
//   Pt                homogeneous projective (X : Y : Z); the identity is (0 : 1 : 0).  pt_add / pt_dbl are the COMPLETE a = -3 formulas of
//                     Renes, Costello and Batina (algorithms 4 and 6): no exceptional case, no branch.
//   nistp_mul         k P for a SECRET k and a SECRET P: one doubling and one addition per scalar bit from the top, the addend chosen
//                     between P and the identity by per-lane selects.  No table: nothing secret is addressed or stored.
//   nistp_decode      SEC 1 2.3.4, compressed form only, STRICT: a prefix other than 02 / 03, x >= p and a non-residue x^3 - 3x + b all give
//                     verdict 0.  The all-zero row is the identity (the reference's one-byte 00, padded).  Computes either way.
//   sswu_map          group/short.go sswu3mod4Map step by step, e1 (xd = 0 -> Z A) and both selects included; sgn0 is the low bit of the
//                     canonical value.  The result stays projective (xn : y xd : xd): the reference's inversion of xd is not needed.
//   (hashing)         expand_message_xmd is hkdf::xmd of hkdf_stream_dev.h: L and 2 L bytes need 2 and 3 digests.
//
// Constant time: no branch and no address depends on a scalar, a blind, a key, a hashed point or an evaluated element.  Only lengths and
// public exponents steer loops.
#pragma once
#include <stdint.h>

#include "hkdf_stream_dev.h"

// The Montgomery product is a function of its own on the device: a point addition and a doubling are 27 of them, and inlined the loop body
// of a multiplication would be tens of kilobytes of straight-line code per curve.  Operands and result travel as vectors of N words: the
// calling convention passes a vector in registers, where two structs of twelve words would go through the stack.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CIRCL_NISTP_INLINE_MUL)
#define CIRCL_NISTP_MUL_CALL 1
#else
#define CIRCL_NISTP_MUL_CALL 0
#endif

namespace circl {
namespace nistp {

using sha512::bswap32;

template <int N>
struct Fe {
    uint32_t v[N];
};

// ---- the curve descriptions ---------------------------------------------------------------------------------------------------------
#define NISTP_WORDS(NAME, ...)                    \
    static CIRCL_HD uint32_t NAME(int i) {        \
        constexpr uint32_t w[N] = {__VA_ARGS__};  \
        return w[i];                              \
    }

struct P256 {
    static constexpr int N = 8, BITS = 256, L = 48, NS = 32, NE = 33, CURVE = 256;
    using Hash = hkdf::Sha256;
    struct Fp {  // p = 2^256 - 2^224 + 2^192 + 2^96 - 1
        static constexpr int N = 8;
        static constexpr uint32_t NINV = 1u;  // -p^-1 mod 2^32: p = -1 mod 2^32
        NISTP_WORDS(mod, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu)
        NISTP_WORDS(one, 0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u)  // R mod p
        NISTP_WORDS(rr, 0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u)   // R^2
        NISTP_WORDS(rrr, 0x0000000au, 0xfffffffdu, 0xfffffff7u, 0xffffffedu, 0xfffffffcu, 0x00000005u, 0x00000001u, 0x00000018u)  // R^3
    };
    struct Fn {  // the order of the group
        static constexpr int N = 8;
        static constexpr uint32_t NINV = 0xee00bc4fu;
        NISTP_WORDS(mod, 0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu)
        NISTP_WORDS(one, 0x039cdaafu, 0x0c46353du, 0x58e8617bu, 0x43190552u, 0x00000000u, 0x00000000u, 0xffffffffu, 0x00000000u)
        NISTP_WORDS(rr, 0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu, 0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u)
        NISTP_WORDS(rrr, 0x0b65a624u, 0xac8ebec9u, 0x0c0555c9u, 0x111f28aeu, 0x6ba5e93fu, 0x2543b924u, 0x6407be65u, 0x503a54e7u)
    };
    // Montgomery forms mod p: b, Z = -10, Z A = 30, c2 = sqrt(-Z^3) (group/short.go:404-426), the generator
    NISTP_WORDS(b, 0x29c4bddfu, 0xd89cdf62u, 0x78843090u, 0xacf005cdu, 0xf7212ed6u, 0xe5a220abu, 0x04874834u, 0xdc30061du)
    NISTP_WORDS(z, 0xfffffff5u, 0xffffffffu, 0xffffffffu, 0x0000000au, 0x00000000u, 0x00000000u, 0x0000000bu, 0xfffffff5u)
    NISTP_WORDS(za, 0x0000001eu, 0x00000000u, 0x00000000u, 0xffffffe2u, 0xffffffffu, 0xffffffffu, 0xffffffe1u, 0x0000001du)
    NISTP_WORDS(c2, 0x09b02418u, 0xac1bc6aeu, 0x6995e599u, 0x4d7f939du, 0xcd6740afu, 0xe53a2a63u, 0x456681d9u, 0x5ccdc7adu)
    NISTP_WORDS(gx, 0x18a9143cu, 0x79e730d4u, 0x5fedb601u, 0x75ba95fcu, 0x77622510u, 0x79fb732bu, 0xa53755c6u, 0x18905f76u)
    NISTP_WORDS(gy, 0xce95560au, 0xddf25357u, 0xba19e45cu, 0x8b4ab8e4u, 0xdd21f325u, 0xd2e88688u, 0x25885d85u, 0x8571ff18u)
};

struct P384 {
    static constexpr int N = 12, BITS = 384, L = 72, NS = 48, NE = 49, CURVE = 384;
    using Hash = hkdf::Sha384;
    struct Fp {  // p = 2^384 - 2^128 - 2^96 + 2^32 - 1
        static constexpr int N = 12;
        static constexpr uint32_t NINV = 1u;  // -p^-1 mod 2^32: p = -1 mod 2^32
        NISTP_WORDS(mod, 0xffffffffu, 0x00000000u, 0x00000000u, 0xffffffffu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                    0xffffffffu, 0xffffffffu)
        NISTP_WORDS(one, 0x00000001u, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
                    0x00000000u, 0x00000000u)
        NISTP_WORDS(rr, 0x00000001u, 0xfffffffeu, 0x00000000u, 0x00000002u, 0x00000000u, 0xfffffffeu, 0x00000000u, 0x00000002u, 0x00000001u, 0x00000000u,
                    0x00000000u, 0x00000000u)
        NISTP_WORDS(rrr, 0x00000002u, 0xfffffffcu, 0x00000002u, 0x00000003u, 0xfffffffeu, 0xfffffffcu, 0x00000005u, 0x00000003u, 0xfffffffdu, 0xfffffffdu,
                    0x00000002u, 0x00000003u)
    };
    struct Fn {
        static constexpr int N = 12;
        static constexpr uint32_t NINV = 0xe88fdc45u;
        NISTP_WORDS(mod, 0xccc52973u, 0xecec196au, 0x48b0a77au, 0x581a0db2u, 0xf4372ddfu, 0xc7634d81u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                    0xffffffffu, 0xffffffffu)
        NISTP_WORDS(one, 0x333ad68du, 0x1313e695u, 0xb74f5885u, 0xa7e5f24du, 0x0bc8d220u, 0x389cb27eu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
                    0x00000000u, 0x00000000u)
        NISTP_WORDS(rr, 0x19b409a9u, 0x2d319b24u, 0xdf1aa419u, 0xff3d81e5u, 0xfcb82947u, 0xbc3e483au, 0x4aab1cc5u, 0xd40d4917u, 0x28266895u, 0x3fb05b7au,
                    0x2b39bf21u, 0x0c84ee01u)
        NISTP_WORDS(rrr, 0x377c7677u, 0x302a6fafu, 0xd26894bcu, 0x2a70cb61u, 0xba8dc4bau, 0x0c27ddb8u, 0xedb48eb6u, 0x5dbd3f41u, 0x9522617bu, 0x16d08167u,
                    0xb33c33c6u, 0xd558bfbcu)
    };
    // Montgomery forms mod p: b, Z = -12, Z A = 36, c2 = sqrt(-Z^3), the generator
    NISTP_WORDS(b, 0x9d412dccu, 0x08118871u, 0x7a4c32ecu, 0xf729add8u, 0x1920022eu, 0x77f2209bu, 0x94938ae2u, 0xe3374beeu, 0x1f022094u, 0xb62b21f4u,
                0x604fbff9u, 0xcd08114bu)
    NISTP_WORDS(z, 0xfffffff3u, 0x0000000cu, 0x00000000u, 0xfffffff3u, 0xfffffff2u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                0xffffffffu, 0xffffffffu)
    NISTP_WORDS(za, 0x00000024u, 0xffffffdcu, 0xffffffffu, 0x00000023u, 0x00000024u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
                0x00000000u, 0x00000000u)
    NISTP_WORDS(c2, 0x07af57aau, 0x5a79354fu, 0x906b8b55u, 0xe75a4ed1u, 0xf122de6du, 0x7588d991u, 0x5904d48eu, 0x186bd88fu, 0x06efdb00u, 0xb1e7aa2du,
                0xc2b08b2au, 0x1abba906u)
    NISTP_WORDS(gx, 0x49c0b528u, 0x3dd07566u, 0xa0d6ce38u, 0x20e378e2u, 0x541b4d6eu, 0x879c3afcu, 0x59a30effu, 0x64548684u, 0x614ede2bu, 0x812ff723u,
                0x299e1513u, 0x4d3aadc2u)
    NISTP_WORDS(gy, 0x4b03a4feu, 0x23043dadu, 0x7bb4a9acu, 0xa1bfa8bfu, 0x2e83b050u, 0x8bade756u, 0x68f4ffd9u, 0xc6c35219u, 0x3969a840u, 0xdd800226u,
                0x5a15c5e9u, 0x2b78abc2u)
};
#undef NISTP_WORDS

// ---- arithmetic modulo M::mod (p or n), N limbs, every value below the modulus ------------------------------------------------------
template <class M, class F>
CIRCL_HD Fe<M::N> fe_lit(F word) {  // a constant of a description: fe_lit<Fp>(C::b)
    Fe<M::N> r;
#pragma unroll
    for (int i = 0; i < M::N; i++) r.v[i] = word(i);
    return r;
}
template <class M>
CIRCL_HD Fe<M::N> fe_zero() {
    Fe<M::N> r;
#pragma unroll
    for (int i = 0; i < M::N; i++) r.v[i] = 0;
    return r;
}
template <class M>
CIRCL_HD Fe<M::N> fe_one() { return fe_lit<M>(M::one); }  // 1 in Montgomery form

// t (N words and a carry word hi in {0, 1}) below twice the modulus: t - m where t >= m, else t
template <class M>
CIRCL_HD Fe<M::N> sub_mod_if_ge(const uint32_t *t, uint32_t hi) {
    constexpr int N = M::N;
    uint32_t d[N], borrow = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint64_t x = (uint64_t)t[i] - M::mod(i) - borrow;
        d[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 63);
    }
    const uint32_t take = 0u - (hi | (borrow ^ 1u));  // all ones iff t >= m
    Fe<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.v[i] = (d[i] & take) | (t[i] & ~take);
    return r;
}

template <class M>
CIRCL_HD Fe<M::N> fe_add(const Fe<M::N> &a, const Fe<M::N> &b) {
    constexpr int N = M::N;
    uint32_t s[N], carry = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint64_t x = (uint64_t)a.v[i] + b.v[i] + carry;
        s[i] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
    return sub_mod_if_ge<M>(s, carry);
}
template <class M>
CIRCL_HD Fe<M::N> fe_sub(const Fe<M::N> &a, const Fe<M::N> &b) {
    constexpr int N = M::N;
    uint32_t d[N], borrow = 0, carry = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint64_t x = (uint64_t)a.v[i] - b.v[i] - borrow;
        d[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 63);
    }
    const uint32_t wrap = 0u - borrow;  // a < b: add the modulus back
    Fe<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint64_t x = (uint64_t)d[i] + (M::mod(i) & wrap) + carry;
        r.v[i] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
    return r;
}
template <class M>
CIRCL_HD Fe<M::N> fe_neg(const Fe<M::N> &a) { return fe_sub<M>(fe_zero<M>(), a); }
template <int N>
CIRCL_HD Fe<N> fe_select(const Fe<N> &a, const Fe<N> &b, bool take_b) {  // take_b ? b : a, by masks
    const uint32_t m = 0u - (uint32_t)take_b;
    Fe<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.v[i] = (a.v[i] & ~m) | (b.v[i] & m);
    return r;
}
template <int N>
CIRCL_HD bool fe_is_zero(const Fe<N> &a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < N; i++) o |= a.v[i];
    return o == 0;
}
template <int N>
CIRCL_HD bool fe_equal(const Fe<N> &a, const Fe<N> &b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < N; i++) o |= a.v[i] ^ b.v[i];
    return o == 0;
}
// 1 iff the plain value a is below the modulus
template <class M>
CIRCL_HD uint32_t fe_is_canonical(const Fe<M::N> &a) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < M::N; i++) {
        const uint64_t x = (uint64_t)a.v[i] - M::mod(i) - borrow;
        borrow = (uint32_t)(x >> 63);
    }
    return borrow;
}

// a b / R mod m for a below R and b below m (or the other way round): the result is below m.  Row i adds a b[i], then q m with
// q = t[0] NINV, which clears the low limb, and shifts down by one limb.
template <class M>
CIRCL_HD Fe<M::N> mont_mul_body(const Fe<M::N> &a, const Fe<M::N> &b) {
    constexpr int N = M::N;
    uint32_t t[N + 2];
#pragma unroll
    for (int j = 0; j < N + 2; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t uv = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
            t[j] = (uint32_t)uv;
            c = uv >> 32;
        }
        uint64_t uv = (uint64_t)t[N] + c;
        t[N] = (uint32_t)uv;
        t[N + 1] = (uint32_t)(uv >> 32);
        const uint32_t q = t[0] * M::NINV;
        c = ((uint64_t)q * M::mod(0) + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < N; j++) {
            uv = (uint64_t)q * M::mod(j) + t[j] + c;
            t[j - 1] = (uint32_t)uv;
            c = uv >> 32;
        }
        uv = (uint64_t)t[N] + c;
        t[N - 1] = (uint32_t)uv;
        t[N] = t[N + 1] + (uint32_t)(uv >> 32);
    }
    return sub_mod_if_ge<M>(t, t[N]);
}
#if CIRCL_NISTP_MUL_CALL
template <int N>
using Vec = uint32_t __attribute__((ext_vector_type(N)));
template <class M>
static __device__ __attribute__((noinline)) Vec<M::N> mont_mul_call(Vec<M::N> a, Vec<M::N> b) {
    Fe<M::N> x, y;
#pragma unroll
    for (int i = 0; i < M::N; i++) {
        x.v[i] = a[i];
        y.v[i] = b[i];
    }
    const Fe<M::N> r = mont_mul_body<M>(x, y);
    Vec<M::N> o;
#pragma unroll
    for (int i = 0; i < M::N; i++) o[i] = r.v[i];
    return o;
}
template <class M>
CIRCL_HD Fe<M::N> mont_mul(const Fe<M::N> &a, const Fe<M::N> &b) {
    Vec<M::N> x, y;
#pragma unroll
    for (int i = 0; i < M::N; i++) {
        x[i] = a.v[i];
        y[i] = b.v[i];
    }
    const Vec<M::N> o = mont_mul_call<M>(x, y);
    Fe<M::N> r;
#pragma unroll
    for (int i = 0; i < M::N; i++) r.v[i] = o[i];
    return r;
}
#else
template <class M>
CIRCL_HD Fe<M::N> mont_mul(const Fe<M::N> &a, const Fe<M::N> &b) { return mont_mul_body<M>(a, b); }
#endif
template <class M>
CIRCL_HD Fe<M::N> mont_sqr(const Fe<M::N> &a) { return mont_mul<M>(a, a); }
template <class M>
CIRCL_HD Fe<M::N> to_mont(const Fe<M::N> &a) { return mont_mul<M>(a, fe_lit<M>(M::rr)); }  // a below R
template <class M>
CIRCL_HD Fe<M::N> from_mont(const Fe<M::N> &a) {
    Fe<M::N> one = fe_zero<M>();
    one.v[0] = 1;
    return mont_mul<M>(a, one);
}

// x^e in Montgomery form for the public exponent e = word(0) + 2^32 word(1) + ... of `bits` bits: a squaring per bit from the top and
// a product where the bit is set
template <class M, class F>
CIRCL_HD Fe<M::N> mont_pow(const Fe<M::N> &x, F word, int bits) {
    Fe<M::N> r = fe_one<M>();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = bits - 1; t >= 0; t--) {
        r = mont_sqr<M>(r);
        if ((word(t >> 5) >> (t & 31)) & 1u) r = mont_mul<M>(r, x);
    }
    return r;
}

// ---- GF(p) --------------------------------------------------------------------------------------------------------------------------
// x^((p - 3) / 4): the exponent is p >> 2, since p = 3 mod 4
template <class C>
CIRCL_HD Fe<C::N> fe_pow_c1(const Fe<C::N> &x) {
    using Fp = typename C::Fp;
    return mont_pow<Fp>(x, [](int i) { return (Fp::mod(i) >> 2) | (i + 1 < C::N ? Fp::mod(i + 1) << 30 : 0u); }, C::BITS - 2);
}
// x^((p + 1) / 4) = x x^c1: a square root of x where x is a square (p = 3 mod 4); the caller checks
template <class C>
CIRCL_HD Fe<C::N> fe_sqrt_candidate(const Fe<C::N> &x) { return mont_mul<typename C::Fp>(x, fe_pow_c1<C>(x)); }
// x^(p - 2) = (x^c1)^4 x: the inverse, and 0 for 0
template <class C>
CIRCL_HD Fe<C::N> fe_inv(const Fe<C::N> &x) {
    using Fp = typename C::Fp;
    return mont_mul<Fp>(mont_sqr<Fp>(mont_sqr<Fp>(fe_pow_c1<C>(x))), x);
}
// sgn0 of RFC 9380 4.1 for m = 1: the low bit of the canonical value
template <class C>
CIRCL_HD uint32_t fe_sgn0(const Fe<C::N> &x) { return from_mont<typename C::Fp>(x).v[0] & 1u; }

// ---- scalars mod n: plain little-endian limbs ---------------------------------------------------------------------------------------
template <class C>
CIRCL_HD uint32_t sc_is_canonical(const Fe<C::N> &k) { return fe_is_canonical<typename C::Fn>(k); }
template <class C>
CIRCL_HD bool sc_is_zero(const Fe<C::N> &k) { return fe_is_zero(k); }
template <class C>
CIRCL_HD Fe<C::N> sc_mul(const Fe<C::N> &a, const Fe<C::N> &b) {  // a, b below n
    using Fn = typename C::Fn;
    return mont_mul<Fn>(mont_mul<Fn>(a, b), fe_lit<Fn>(Fn::rr));
}
// x^(n - 2) mod n for x below n.  n - 2: the low word of either order ends in ...1 or ...3 above 2, so no borrow leaves it.
template <class C>
CIRCL_HD Fe<C::N> sc_inv(const Fe<C::N> &x) {
    using Fn = typename C::Fn;
    const Fe<C::N> r = mont_pow<Fn>(to_mont<Fn>(x), [](int i) { return Fn::mod(i) - (i == 0 ? 2u : 0u); }, C::BITS);
    return from_mont<Fn>(r);
}

// the L-byte big-endian string at bytes [at, at + L) of u (words as memory holds them; at a multiple of 4) modulo M::mod, in Montgomery
// form: the value is lo + hi R with lo the low N limbs, and lo R + hi R^2 = mont_mul(lo, R^2) + mont_mul(hi, R^3)
template <class C, class M>
CIRCL_HD Fe<C::N> reduce_wide(const uint32_t *u, int at) {
    constexpr int N = C::N, W = C::L / 4;
    static_assert(C::L % 4 == 0 && W > N && W <= 2 * N, "one limb row above R");
    Fe<N> lo, hi = fe_zero<M>();
#pragma unroll
    for (int i = 0; i < N; i++) lo.v[i] = bswap32(u[at / 4 + W - 1 - i]);
#pragma unroll
    for (int i = N; i < W; i++) hi.v[i - N] = bswap32(u[at / 4 + W - 1 - i]);
    return fe_add<M>(mont_mul<M>(lo, fe_lit<M>(M::rr)), mont_mul<M>(hi, fe_lit<M>(M::rrr)));
}

// a row of NS big-endian bytes held as N words of memory <-> the plain limbs
template <class C>
CIRCL_HD Fe<C::N> sc_load(const uint32_t *row) {
    Fe<C::N> k;
#pragma unroll
    for (int i = 0; i < C::N; i++) k.v[i] = bswap32(row[C::N - 1 - i]);
    return k;
}
template <class C>
CIRCL_HD void sc_store(uint32_t *row, const Fe<C::N> &k, uint32_t good) {
    const uint32_t mask = 0u - good;
#pragma unroll
    for (int i = 0; i < C::N; i++) row[C::N - 1 - i] = bswap32(k.v[i]) & mask;
}

// ---- points -------------------------------------------------------------------------------------------------------------------------
template <class C>
struct Pt {
    Fe<C::N> X, Y, Z;
};
template <class C>
CIRCL_HD Pt<C> pt_identity() {
    return {fe_zero<typename C::Fp>(), fe_one<typename C::Fp>(), fe_zero<typename C::Fp>()};
}
template <class C>
CIRCL_HD Pt<C> pt_generator() {
    using Fp = typename C::Fp;
    return {fe_lit<Fp>(C::gx), fe_lit<Fp>(C::gy), fe_one<Fp>()};
}
template <class C>
CIRCL_HD Pt<C> pt_select(const Pt<C> &a, const Pt<C> &b, bool take_b) {
    return {fe_select(a.X, b.X, take_b), fe_select(a.Y, b.Y, take_b), fe_select(a.Z, b.Z, take_b)};
}
template <class C>
CIRCL_HD bool pt_is_identity(const Pt<C> &p) { return fe_is_zero(p.Z); }
// a point as 3 N words, X || Y || Z: what a lane hands to another lane or to a workspace
template <class C>
CIRCL_HD void pt_store(uint32_t *w, const Pt<C> &p) {
#pragma unroll
    for (int i = 0; i < C::N; i++) {
        w[i] = p.X.v[i];
        w[C::N + i] = p.Y.v[i];
        w[2 * C::N + i] = p.Z.v[i];
    }
}
template <class C>
CIRCL_HD Pt<C> pt_load(const uint32_t *w) {
    Pt<C> p;
#pragma unroll
    for (int i = 0; i < C::N; i++) {
        p.X.v[i] = w[i];
        p.Y.v[i] = w[C::N + i];
        p.Z.v[i] = w[2 * C::N + i];
    }
    return p;
}

// eprint 2015/1060 algorithm 4: the complete addition for a = -3, 12 products and 2 by b
template <class C>
CIRCL_HD Pt<C> pt_add(const Pt<C> &p, const Pt<C> &q) {
    using M = typename C::Fp;
    const Fe<C::N> b = fe_lit<M>(C::b);
    Fe<C::N> t0 = mont_mul<M>(p.X, q.X), t1 = mont_mul<M>(p.Y, q.Y), t2 = mont_mul<M>(p.Z, q.Z);
    Fe<C::N> t3 = fe_add<M>(p.X, p.Y), t4 = fe_add<M>(q.X, q.Y), X3, Y3, Z3;
    t3 = mont_mul<M>(t3, t4);
    t4 = fe_add<M>(t0, t1);
    t3 = fe_sub<M>(t3, t4);
    t4 = fe_add<M>(p.Y, p.Z);
    X3 = fe_add<M>(q.Y, q.Z);
    t4 = mont_mul<M>(t4, X3);
    X3 = fe_add<M>(t1, t2);
    t4 = fe_sub<M>(t4, X3);
    X3 = fe_add<M>(p.X, p.Z);
    Y3 = fe_add<M>(q.X, q.Z);
    X3 = mont_mul<M>(X3, Y3);
    Y3 = fe_add<M>(t0, t2);
    Y3 = fe_sub<M>(X3, Y3);
    Z3 = mont_mul<M>(b, t2);
    X3 = fe_sub<M>(Y3, Z3);
    Z3 = fe_add<M>(X3, X3);
    X3 = fe_add<M>(X3, Z3);
    Z3 = fe_sub<M>(t1, X3);
    X3 = fe_add<M>(t1, X3);
    Y3 = mont_mul<M>(b, Y3);
    t1 = fe_add<M>(t2, t2);
    t2 = fe_add<M>(t1, t2);
    Y3 = fe_sub<M>(Y3, t2);
    Y3 = fe_sub<M>(Y3, t0);
    t1 = fe_add<M>(Y3, Y3);
    Y3 = fe_add<M>(t1, Y3);
    t1 = fe_add<M>(t0, t0);
    t0 = fe_add<M>(t1, t0);
    t0 = fe_sub<M>(t0, t2);
    t1 = mont_mul<M>(t4, Y3);
    t2 = mont_mul<M>(t0, Y3);
    Y3 = mont_mul<M>(X3, Z3);
    Y3 = fe_add<M>(Y3, t2);
    X3 = mont_mul<M>(t3, X3);
    X3 = fe_sub<M>(X3, t1);
    Z3 = mont_mul<M>(t4, Z3);
    t1 = mont_mul<M>(t3, t0);
    Z3 = fe_add<M>(Z3, t1);
    return {X3, Y3, Z3};
}

// eprint 2015/1060 algorithm 6: the complete doubling for a = -3
template <class C>
CIRCL_HD Pt<C> pt_dbl(const Pt<C> &p) {
    using M = typename C::Fp;
    const Fe<C::N> b = fe_lit<M>(C::b);
    Fe<C::N> t0 = mont_sqr<M>(p.X), t1 = mont_sqr<M>(p.Y), t2 = mont_sqr<M>(p.Z), t3 = mont_mul<M>(p.X, p.Y), X3, Y3, Z3;
    t3 = fe_add<M>(t3, t3);
    Z3 = mont_mul<M>(p.X, p.Z);
    Z3 = fe_add<M>(Z3, Z3);
    Y3 = mont_mul<M>(b, t2);
    Y3 = fe_sub<M>(Y3, Z3);
    X3 = fe_add<M>(Y3, Y3);
    Y3 = fe_add<M>(X3, Y3);
    X3 = fe_sub<M>(t1, Y3);
    Y3 = fe_add<M>(t1, Y3);
    Y3 = mont_mul<M>(X3, Y3);
    X3 = mont_mul<M>(X3, t3);
    t3 = fe_add<M>(t2, t2);
    t2 = fe_add<M>(t2, t3);
    Z3 = mont_mul<M>(b, Z3);
    Z3 = fe_sub<M>(Z3, t2);
    Z3 = fe_sub<M>(Z3, t0);
    t3 = fe_add<M>(Z3, Z3);
    Z3 = fe_add<M>(Z3, t3);
    t3 = fe_add<M>(t0, t0);
    t0 = fe_add<M>(t3, t0);
    t0 = fe_sub<M>(t0, t2);
    t0 = mont_mul<M>(t0, Z3);
    Y3 = fe_add<M>(Y3, t0);
    t0 = mont_mul<M>(p.Y, p.Z);
    t0 = fe_add<M>(t0, t0);
    Z3 = mont_mul<M>(t0, Z3);
    X3 = fe_sub<M>(X3, Z3);
    Z3 = mont_mul<M>(t0, t1);
    Z3 = fe_add<M>(Z3, Z3);
    Z3 = fe_add<M>(Z3, Z3);
    return {X3, Y3, Z3};
}

// k P for a plain k of BITS bits, k and P secret: BITS doublings and BITS additions of P or of the identity, chosen by selects
template <class C>
CIRCL_HD Pt<C> nistp_mul(const Fe<C::N> &k_in, const Pt<C> &p) {
    constexpr int N = C::N;
    Fe<N> k = k_in;
    const Pt<C> e = pt_identity<C>();
    Pt<C> r = e;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int t = C::BITS - 1; t >= 0; t--) {
        const bool bit = (k.v[N - 1] >> 31) != 0;  // the current bit is always the top bit of k
#pragma unroll
        for (int i = N - 1; i > 0; i--) k.v[i] = (k.v[i] << 1) | (k.v[i - 1] >> 31);
        k.v[0] <<= 1;
        r = pt_add<C>(pt_dbl<C>(r), pt_select<C>(e, p, bit));
    }
    return r;
}
template <class C>
CIRCL_HD Pt<C> nistp_base(const Fe<C::N> &k) { return nistp_mul<C>(k, pt_generator<C>()); }

// ---- SEC 1 compressed points: rows of NE bytes held as EW words of memory -----------------------------------------------------------
template <class C>
constexpr int elem_words() { return (C::NE + 3) / 4; }

// SEC 1 2.3.3: 02 | 03 || x, the words as memory holds them; the identity encodes as the zero row.  Returns 1 for the identity.
template <class C>
CIRCL_HD uint32_t nistp_encode(uint32_t *enc, const Pt<C> &p) {
    using Fp = typename C::Fp;
    constexpr int N = C::N, EW = elem_words<C>();
    const Fe<N> zinv = fe_inv<C>(p.Z);  // 0 for the identity: x = y = 0
    const Fe<N> x = from_mont<Fp>(mont_mul<Fp>(p.X, zinv)), y = from_mont<Fp>(mont_mul<Fp>(p.Y, zinv));
    const uint32_t ident = fe_is_zero(p.Z) ? 1u : 0u;
#pragma unroll
    for (int j = 0; j < EW; j++) enc[j] = 0;
    enc[0] = (2u + (y.v[0] & 1u)) & (ident - 1u);
#pragma unroll
    for (int j = 0; j < C::NS; j++) {  // byte 1 + j of the row is byte NS - 1 - j of x
        const int src = C::NS - 1 - j, dst = 1 + j;
        enc[dst / 4] |= ((x.v[src / 4] >> (8 * (src % 4))) & 0xffu) << (8 * (dst % 4));
    }
    return ident;
}

// SEC 1 2.3.4 on a row of EW words: the verdict (1: a point of the curve or the zero row) and the point, computed either way.
// *ident (if asked for) is 1 for the zero row.
template <class C>
CIRCL_HD uint32_t nistp_decode(Pt<C> &p, const uint32_t *enc, uint32_t *ident = nullptr) {
    using Fp = typename C::Fp;
    constexpr int N = C::N;
    Fe<N> x = fe_zero<Fp>();
#pragma unroll
    for (int j = 0; j < C::NS; j++) {
        const int dst = C::NS - 1 - j, src = 1 + j;
        x.v[dst / 4] |= ((enc[src / 4] >> (8 * (src % 4))) & 0xffu) << (8 * (dst % 4));
    }
    const uint32_t prefix = enc[0] & 0xffu;
    const bool zero_row = prefix == 0 && fe_is_zero(x);
    const uint32_t in_range = fe_is_canonical<Fp>(x);
    const Fe<N> xm = to_mont<Fp>(x), one = fe_one<Fp>();
    // y^2 = x^3 - 3 x + b
    const Fe<N> x3 = fe_add<Fp>(fe_add<Fp>(xm, xm), xm);
    const Fe<N> rhs = fe_add<Fp>(fe_sub<Fp>(mont_mul<Fp>(mont_sqr<Fp>(xm), xm), x3), fe_lit<Fp>(C::b));
    Fe<N> y = fe_sqrt_candidate<C>(rhs);
    const bool is_square = fe_equal(mont_sqr<Fp>(y), rhs);
    y = fe_select(y, fe_neg<Fp>(y), fe_sgn0<C>(y) != (prefix & 1u));
    const Pt<C> affine = {xm, y, one};
    p = pt_select<C>(affine, pt_identity<C>(), zero_row);
    if (ident) *ident = zero_row ? 1u : 0u;
    return (zero_row || ((prefix | 1u) == 3u && in_range && is_square)) ? 1u : 0u;
}

// rows of NE bytes in global memory, no alignment: read and written bytewise
template <class C>
CIRCL_HD void elem_load(uint32_t *enc, const uint8_t *row) {
    constexpr int EW = elem_words<C>();
#pragma unroll
    for (int j = 0; j < EW; j++) enc[j] = 0;
#pragma unroll
    for (int j = 0; j < C::NE; j++) enc[j / 4] |= (uint32_t)row[j] << (8 * (j % 4));
}
template <class C>
CIRCL_HD void elem_store(uint8_t *row, const uint32_t *enc, uint32_t good) {
    const uint32_t mask = 0u - good;
#pragma unroll
    for (int j = 0; j < C::NE; j++) row[j] = (uint8_t)((enc[j / 4] & mask) >> (8 * (j % 4)));
}

// ---- hashing ------------------------------------------------------------------------------------------------------------------------
// group/short.go:428-503 sswu3mod4Map on u in Montgomery form, the step numbers are the reference's.  Returns (xn : y xd : xd).
template <class C>
CIRCL_HD Pt<C> sswu_map(const Fe<C::N> &u) {
    using M = typename C::Fp;
    constexpr int N = C::N;
    const Fe<N> B = fe_lit<M>(C::b), Z = fe_lit<M>(C::z);
    const Fe<N> tv1 = mont_sqr<M>(u);                                        // 1
    const Fe<N> tv3 = mont_mul<M>(Z, tv1);                                   // 2
    Fe<N> tv2 = mont_sqr<M>(tv3);                                            // 3
    Fe<N> xd = fe_add<M>(tv2, tv3);                                          // 4
    const Fe<N> x1n = mont_mul<M>(fe_add<M>(xd, fe_one<M>()), B);            // 5, 6
    xd = fe_add<M>(fe_add<M>(xd, xd), xd);                                   // 7: -A xd = 3 xd
    const bool e1 = fe_is_zero(xd);                                          // 8
    xd = fe_select(xd, fe_lit<M>(C::za), e1);                                // 9
    tv2 = mont_sqr<M>(xd);                                                   // 10
    const Fe<N> gxd = mont_mul<M>(tv2, xd);                                  // 11
    tv2 = fe_neg<M>(fe_add<M>(fe_add<M>(tv2, tv2), tv2));                    // 12: A tv2 = -3 tv2
    Fe<N> gx1 = fe_add<M>(mont_sqr<M>(x1n), tv2);                            // 13, 14
    gx1 = mont_mul<M>(gx1, x1n);                                             // 15
    gx1 = fe_add<M>(gx1, mont_mul<M>(B, gxd));                               // 16, 17
    Fe<N> tv4 = mont_sqr<M>(gxd);                                            // 18
    tv2 = mont_mul<M>(gx1, gxd);                                             // 19
    tv4 = mont_mul<M>(tv4, tv2);                                             // 20
    const Fe<N> y1 = mont_mul<M>(fe_pow_c1<C>(tv4), tv2);                    // 21, 22
    const Fe<N> x2n = mont_mul<M>(tv3, x1n);                                 // 23
    const Fe<N> y2 = mont_mul<M>(mont_mul<M>(mont_mul<M>(y1, fe_lit<M>(C::c2)), tv1), u);  // 24, 25, 26
    tv2 = mont_mul<M>(mont_sqr<M>(y1), gxd);                                 // 27, 28
    const bool e2 = fe_equal(tv2, gx1);                                      // 29
    const Fe<N> xn = fe_select(x2n, x1n, e2);                                // 30
    Fe<N> y = fe_select(y2, y1, e2);                                         // 31
    const bool e3 = fe_sgn0<C>(u) == fe_sgn0<C>(y);                          // 32
    y = fe_select(fe_neg<M>(y), y, e3);                                      // 33
    return {xn, mont_mul<M>(y, xd), xd};                                     // 34, projective
}

// the words an xmd of COUNT field elements needs
template <class C, int COUNT>
constexpr int uniform_words() {
    return (COUNT * C::L + C::Hash::OUT - 1) / C::Hash::OUT * (C::Hash::OUT / 4);
}

// group/short.go HashToElement / HashToElementNonUniform on the uniform bytes: two field elements mapped and added, or one mapped
template <class C>
CIRCL_HD Pt<C> nistp_from_uniform(const uint32_t *u, bool nonuniform) {
    using Fp = typename C::Fp;
    const Pt<C> q0 = sswu_map<C>(reduce_wide<C, Fp>(u, 0));
    if (nonuniform) return q0;  // (a launch-wide flag)
    return pt_add<C>(q0, sswu_map<C>(reduce_wide<C, Fp>(u, C::L)));
}
// group/short.go HashToScalar on the uniform bytes: the big-endian value mod n, plain
template <class C>
CIRCL_HD Fe<C::N> sc_from_uniform(const uint32_t *u) {
    using Fn = typename C::Fn;
    return from_mont<Fn>(reduce_wide<C, Fn>(u, 0));
}

}  // namespace nistp
}  // namespace circl
