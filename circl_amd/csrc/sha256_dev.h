// sha256_dev.h -- FIPS 180-4 SHA-256 on gfx950, one message per lane.
//
// Serves the HPKE DHKEM over X25519 (hpke/kembase.go: HKDF-SHA256 through hkdf_dev.h) and the batch primitive
// circl_hip_sha256.  Modelled on sha512_dev.h: a word is one 32-bit register, every rotation of the Sigma / sigma functions is
// a single V_ALIGNBIT_B32 of the word with itself, and Ch / Maj / the three-way XORs are left to the compiler, which reaches
// V_BITOP3_B32 / V_XOR3_B32 on gfx950.
//
// The message of a lane is `head` (0, 32 or 64 bytes the caller holds in registers) followed by `len` bytes at `msg` in global
// memory, read as aligned dwords (the ragged msg_blob / msg_off layout gives no alignment).  Lengths are public; no address or
// branch depends on the bytes.
#pragma once
#include <stdint.h>

#include "sha512_dev.h"  // CIRCL_HD, align32, bswap32, msg_word: the byte plumbing is the same

namespace circl {
namespace sha256 {

using sha512::align32;
using sha512::bswap32;
using sha512::msg_word;

template <int N>
CIRCL_HD uint32_t rotr(uint32_t x) {
    static_assert(N > 0 && N < 32, "rotation");
    return align32(x, x, N);
}
CIRCL_HD uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return (e & f) ^ (~e & g); }
CIRCL_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) ^ (a & c) ^ (b & c); }

CIRCL_HD uint32_t round_const(int t) {  // FIPS 180-4 4.2.2
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[t];
}

struct State {
    uint32_t h[8];
};

CIRCL_HD void init(State &s) {
    constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
    for (int i = 0; i < 8; i++) s.h[i] = IV[i];
}

// one 64-byte block, w[16] its big-endian words (overwritten: the schedule runs in a ring of 16)
CIRCL_HD void compress(State &s, uint32_t w[16]) {
    uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < 64; r += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (r > 0) {  // W_t = sigma1(W_t-2) + W_t-7 + sigma0(W_t-15) + W_t-16
                const uint32_t w2 = w[(i + 14) & 15], w15 = w[(i + 1) & 15];
                const uint32_t s1 = rotr<17>(w2) ^ rotr<19>(w2) ^ (w2 >> 10);
                const uint32_t s0 = rotr<7>(w15) ^ rotr<18>(w15) ^ (w15 >> 3);
                w[i] = w[i] + s1 + w[(i + 9) & 15] + s0;
            }
            const uint32_t t1 = h + (rotr<6>(e) ^ rotr<11>(e) ^ rotr<25>(e)) + ch(e, f, g) + round_const(r + i) + w[i];
            const uint32_t t2 = (rotr<2>(a) ^ rotr<13>(a) ^ rotr<22>(a)) + maj(a, b, c);
            h = g;
            g = f;
            f = e;
            e = d + t1;
            d = c;
            c = b;
            b = a;
            a = t1 + t2;
        }
    }
    s.h[0] += a;
    s.h[1] += b;
    s.h[2] += c;
    s.h[3] += d;
    s.h[4] += e;
    s.h[5] += f;
    s.h[6] += g;
    s.h[7] += h;
}

// SHA-256(head || msg[0 .. len)): head = HEAD_WORDS little-endian 32-bit words (the bytes as they sit in memory), HEAD_WORDS
// in {0, 8, 16}; out = the 32-byte digest as eight little-endian words (the bytes of the digest in order).
template <int HEAD_WORDS>
CIRCL_HD void hash(uint32_t out[8], const uint32_t *head, const uint8_t *msg, uint64_t len) {
    static_assert(HEAD_WORDS == 0 || HEAD_WORDS == 8 || HEAD_WORDS == 16, "head of 0, 32 or 64 bytes");
    constexpr uint64_t HB = 4 * HEAD_WORDS;
    const uint64_t total = HB + len;
    const uint64_t nblocks = (total + 9 + 63) / 64;
    State s;
    init(s);
    for (uint64_t b = 0; b < nblocks; b++) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t p = b * 64 + 4 * (uint64_t)i;  // a 64-byte head fills block 0, a 32-byte one its first half
            if (i < HEAD_WORDS && b == 0) w[i] = bswap32(head[i < HEAD_WORDS ? i : 0]);
            else w[i] = msg_word(msg, len, p - HB);
        }
        if (b == nblocks - 1) {  // the bit length, big-endian in the last 8 bytes
            const uint64_t bits = total << 3;
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
        compress(s, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = bswap32(s.h[i]);
}

}  // namespace sha256
}  // namespace circl
