// sha512_dev.h -- FIPS 180-4 SHA-512 on gfx950, one message per lane.
//
// Serves Ed25519 (sign/ed25519/ed25519.go hashes with crypto/sha512: the key expansion of the seed, the nonce
// SHA-512(prefix || M) and the challenge SHA-512(R || A || M)) and the batch primitive circl_hip_sha512.
//
// A 64-bit word is a pair of 32-bit registers: the rotations of the Sigma functions are two V_ALIGNBIT_B32 each (a
// rotation by n >= 32 swaps the halves first), the shifts of the sigma functions are one V_ALIGNBIT_B32 and one shift,
// and Ch / Maj / the three-way XORs are left to the compiler, which reaches V_BITOP3_B32 / V_XOR3_B32 on gfx950.  The
// 64-bit additions are V_ADD_CO / V_ADDC pairs.
//
// The message of a lane is `head` (0, 32 or 64 bytes the caller holds in registers: a prefix, R || A) followed by `len`
// bytes at `msg` in global memory, read as aligned dwords (the project's ragged msg_blob / msg_off layout gives no
// alignment), so that lanes of one wavefront hash messages of different lengths, as ML-DSA's mu does.  Lengths are
// public; no address or branch depends on the bytes.
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
namespace sha512 {

struct W64 {
    uint32_t lo, hi;
};

// (hi:lo) >> n of the 64-bit concatenation, low word, 0 <= n < 32
CIRCL_HD uint32_t align32(uint32_t hi, uint32_t lo, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, n);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> n);
#endif
}

template <int N>
CIRCL_HD W64 rotr(W64 x) {
    static_assert(N > 0 && N < 64 && N != 32, "rotation");
    if (N < 32) return {align32(x.hi, x.lo, N), align32(x.lo, x.hi, N)};
    return {align32(x.lo, x.hi, N - 32), align32(x.hi, x.lo, N - 32)};
}
template <int N>
CIRCL_HD W64 shr(W64 x) {
    static_assert(N > 0 && N < 32, "shift");
    return {align32(x.hi, x.lo, N), x.hi >> N};
}
CIRCL_HD W64 add(W64 a, W64 b) {
    const uint64_t s = (((uint64_t)a.hi << 32) | a.lo) + (((uint64_t)b.hi << 32) | b.lo);
    return {(uint32_t)s, (uint32_t)(s >> 32)};
}
CIRCL_HD W64 xor3(W64 a, W64 b, W64 c) { return {a.lo ^ b.lo ^ c.lo, a.hi ^ b.hi ^ c.hi}; }
CIRCL_HD W64 ch(W64 e, W64 f, W64 g) { return {(e.lo & f.lo) ^ (~e.lo & g.lo), (e.hi & f.hi) ^ (~e.hi & g.hi)}; }
CIRCL_HD W64 maj(W64 a, W64 b, W64 c) {
    return {(a.lo & b.lo) ^ (a.lo & c.lo) ^ (b.lo & c.lo), (a.hi & b.hi) ^ (a.hi & c.hi) ^ (b.hi & c.hi)};
}

CIRCL_HD W64 round_const(int t) {  // FIPS 180-4 4.2.3
    static constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
        0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
        0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
        0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
        0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
        0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
        0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    return {(uint32_t)K[t], (uint32_t)(K[t] >> 32)};
}

struct State {
    W64 h[8];
};

CIRCL_HD void init(State &s) {
    constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] = {(uint32_t)IV[i], (uint32_t)(IV[i] >> 32)};
}

// one 128-byte block, w[16] its big-endian words
CIRCL_HD void compress(State &s, W64 w[16]) {
    W64 a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < 80; r += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (r > 0) {  // W_t = sigma1(W_t-2) + W_t-7 + sigma0(W_t-15) + W_t-16, in a ring of 16
                const W64 w2 = w[(i + 14) & 15], w15 = w[(i + 1) & 15];
                const W64 s1 = xor3(rotr<19>(w2), rotr<61>(w2), shr<6>(w2));
                const W64 s0 = xor3(rotr<1>(w15), rotr<8>(w15), shr<7>(w15));
                w[i] = add(add(w[i], s1), add(w[(i + 9) & 15], s0));
            }
            const W64 t1 = add(add(add(h, xor3(rotr<14>(e), rotr<18>(e), rotr<41>(e))), add(ch(e, f, g), round_const(r + i))), w[i]);
            const W64 t2 = add(xor3(rotr<28>(a), rotr<34>(a), rotr<39>(a)), maj(a, b, c));
            h = g;
            g = f;
            f = e;
            e = add(d, t1);
            d = c;
            c = b;
            b = a;
            a = add(t1, t2);
        }
    }
    s.h[0] = add(s.h[0], a);
    s.h[1] = add(s.h[1], b);
    s.h[2] = add(s.h[2], c);
    s.h[3] = add(s.h[3], d);
    s.h[4] = add(s.h[4], e);
    s.h[5] = add(s.h[5], f);
    s.h[6] = add(s.h[6], g);
    s.h[7] = add(s.h[7], h);
}

CIRCL_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// big-endian 32-bit word of the padded message at byte q of the message part (q may lie past its end: 0x80, then zeros).
// The bytes are read as the one or two ALIGNED dwords that hold them, joined by V_ALIGNBIT_B32; a dword is read only if it
// holds a byte of the message, so no read leaves the 4-byte-aligned words the message touches.
CIRCL_HD uint32_t msg_word(const uint8_t *msg, uint64_t len, uint64_t q) {
    if (q >= len) return q == len ? 0x80000000u : 0u;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(msg) + q, a = addr & ~(uintptr_t)3, end = reinterpret_cast<uintptr_t>(msg) + len;
    const uint32_t w0 = *reinterpret_cast<const uint32_t *>(a);
    const uint32_t w1 = a + 4 < end ? *reinterpret_cast<const uint32_t *>(a + 4) : 0u;
    uint32_t v = align32(w1, w0, (uint32_t)(addr & 3) * 8);  // msg[q .. q + 4), little-endian
    const uint64_t valid = len - q;
    if (valid < 4) v = (v & ((1u << (8 * valid)) - 1u)) | (0x80u << (8 * valid));
    return bswap32(v);
}

// SHA-512(head || msg[0 .. len)): head = HEAD_WORDS little-endian 32-bit words (the bytes as they sit in memory), HEAD_WORDS
// in {0, 8, 16}; out = the 64-byte digest as sixteen little-endian words (the bytes of the digest in order).
template <int HEAD_WORDS>
CIRCL_HD void hash(uint32_t out[16], const uint32_t *head, const uint8_t *msg, uint64_t len) {
    static_assert(HEAD_WORDS == 0 || HEAD_WORDS == 8 || HEAD_WORDS == 16, "head of 0, 32 or 64 bytes");
    constexpr uint64_t HB = 4 * HEAD_WORDS;
    const uint64_t total = HB + len;
    const uint64_t nblocks = (total + 17 + 127) / 128;
    State s;
    init(s);
    for (uint64_t b = 0; b < nblocks; b++) {
        W64 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint32_t half[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int hw = 2 * i + k;  // half-word index in the block; the head lies in block 0 only
                const uint64_t p = b * 128 + 4 * (uint64_t)hw;
                if (hw < HEAD_WORDS && b == 0) half[k] = bswap32(head[hw < HEAD_WORDS ? hw : 0]);
                else half[k] = msg_word(msg, len, p - HB);
            }
            w[i] = {half[1], half[0]};
        }
        if (b == nblocks - 1) {  // the bit length, big-endian in the last 16 bytes (total < 2^61: the top 64 bits are zero)
            const uint64_t bits = total << 3;
            w[15] = {(uint32_t)bits, (uint32_t)(bits >> 32)};
        }
        compress(s, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        out[2 * i] = bswap32(s.h[i].hi);
        out[2 * i + 1] = bswap32(s.h[i].lo);
    }
}

}  // namespace sha512
}  // namespace circl
