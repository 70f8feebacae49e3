// hkdf_dev.h -- HMAC, HKDF-Extract and one-block HKDF-Expand (RFC 5869) over a hash policy, and on top of them HPKE's
// LabeledExtract / LabeledExpand for a KEM (hpke/kembase.go:52-82), one computation per lane.
//
// Three policies: Sha256 (block 64, output 32; sha256_dev.h), Sha512 (block 128, output 64; sha512_dev.h) and Sha384 (SHA-512's
// compression from its own initial value, output 48; it serves the run-time-length streams of hkdf_stream_dev.h).  Every message here
// has a length known at compile time, so a message is an array of little-endian 32-bit words (the bytes as they sit in memory)
// that full unrolling keeps in registers: labels are constants the compiler folds, register-held words go in with constant
// shifts (put_word), and the padding and the bit length are constants too.  No byte array, no address and no branch depends on
// the data.  The salt of every Extract is empty (the zero key) and every Expand asks for at most one hash output.
#pragma once
#include <stdint.h>

#include "sha256_dev.h"
#include "sha512_dev.h"

// on the host (tests/hostsim) a compression is a call, so that the many fixed-shape messages do not each inline their own copies
#if defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
#define CIRCL_HKDF_BLOCK static __host__ __device__ __attribute__((noinline))
#else
#define CIRCL_HKDF_BLOCK static CIRCL_HD
#endif

namespace circl {
namespace hkdf {

using sha512::bswap32;

struct Sha256 {
    static constexpr int BLOCK = 64, OUT = 32, LEN_BYTES = 8;
    using State = sha256::State;
    static CIRCL_HD void init(State &s) { sha256::init(s); }
    // one block given as BLOCK / 4 little-endian words
    CIRCL_HKDF_BLOCK void block(State &s, const uint32_t *m) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = bswap32(m[i]);
        sha256::compress(s, w);
    }
    static CIRCL_HD void digest(uint32_t *out, const State &s) {
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = bswap32(s.h[i]);
    }
};

struct Sha512 {
    static constexpr int BLOCK = 128, OUT = 64, LEN_BYTES = 16;
    using State = sha512::State;
    static CIRCL_HD void init(State &s) { sha512::init(s); }
    CIRCL_HKDF_BLOCK void block(State &s, const uint32_t *m) {
        sha512::W64 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = {bswap32(m[2 * i + 1]), bswap32(m[2 * i])};
        sha512::compress(s, w);
    }
    static CIRCL_HD void digest(uint32_t *out, const State &s) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            out[2 * i] = bswap32(s.h[i].hi);
            out[2 * i + 1] = bswap32(s.h[i].lo);
        }
    }
};

// FIPS 180-4 5.3.4 / 6.5: SHA-512's compression from another initial value, the first 48 bytes of the state as the digest
struct Sha384 {
    static constexpr int BLOCK = 128, OUT = 48, LEN_BYTES = 16;
    using State = sha512::State;
    static CIRCL_HD void init(State &s) {
        constexpr uint64_t IV[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull, 0x152fecd8f70e5939ull,
                                    0x67332667ffc00b31ull, 0x8eb44a8768581511ull, 0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
#pragma unroll
        for (int i = 0; i < 8; i++) s.h[i] = {(uint32_t)IV[i], (uint32_t)(IV[i] >> 32)};
    }
    CIRCL_HKDF_BLOCK void block(State &s, const uint32_t *m) {
        sha512::W64 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = {bswap32(m[2 * i + 1]), bswap32(m[2 * i])};
        sha512::compress(s, w);
    }
    static CIRCL_HD void digest(uint32_t *out, const State &s) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            out[2 * i] = bswap32(s.h[i].hi);
            out[2 * i + 1] = bswap32(s.h[i].lo);
        }
    }
};

// blocks / words of the padded message that follows the key block of an HMAC
template <class H>
constexpr int msg_blocks(int len) {
    return (len + 1 + H::LEN_BYTES + H::BLOCK - 1) / H::BLOCK;
}
template <class H>
constexpr int msg_words(int len) {
    return msg_blocks<H>(len) * H::BLOCK / 4;
}

// OR the little-endian word v into the message at byte `off`; off is a constant once the caller's loop is unrolled
CIRCL_HD void put_word(uint32_t *m, int off, uint32_t v) {
    const int i = off / 4, s = 8 * (off % 4);
    m[i] |= v << s;
    if (s) m[i + 1] |= v >> (32 - s);
}
template <int N>
CIRCL_HD void put_bytes(uint32_t *m, int off, const char (&c)[N]) {  // the N - 1 characters of a literal
#pragma unroll
    for (int k = 0; k < N - 1; k++) m[(off + k) / 4] |= (uint32_t)(uint8_t)c[k] << (8 * ((off + k) % 4));
}

// HMAC(key, msg): m = msg_words<H>(LEN) words holding the LEN message bytes and zeros behind them (overwritten: the padding goes
// in here).  ZERO_KEY: the key of an Extract with the empty salt; otherwise key = H::OUT / 4 words.  The two key blocks are
// compressed when they are needed, so that the outer one does not live across the inner hash.
template <class H, int LEN, bool ZERO_KEY>
CIRCL_HD void hmac(uint32_t *out, const uint32_t *key, uint32_t *m) {
    constexpr int NB = msg_blocks<H>(LEN), NW = msg_words<H>(LEN), BW = H::BLOCK / 4, OW = H::OUT / 4;
    static_assert(OW + 1 + H::LEN_BYTES / 4 <= BW, "the outer message is one block");
    m[LEN / 4] |= 0x80u << (8 * (LEN % 4));
    m[NW - 1] = bswap32((uint32_t)(H::BLOCK + LEN) * 8u);
    uint32_t kb[BW];
#pragma unroll
    for (int i = 0; i < BW; i++) kb[i] = ((!ZERO_KEY && i < OW) ? key[i < OW ? i : 0] : 0u) ^ 0x36363636u;
    typename H::State s;
    H::init(s);
    H::block(s, kb);
#pragma unroll
    for (int b = 0; b < NB; b++) H::block(s, m + b * BW);
    uint32_t d[BW];
#pragma unroll
    for (int i = 0; i < BW; i++) d[i] = 0;
    H::digest(d, s);
    d[OW] = 0x80u;
    d[BW - 1] = bswap32((uint32_t)(H::BLOCK + H::OUT) * 8u);
#pragma unroll
    for (int i = 0; i < BW; i++) kb[i] = ((!ZERO_KEY && i < OW) ? key[i < OW ? i : 0] : 0u) ^ 0x5c5c5c5cu;
    H::init(s);
    H::block(s, kb);
    H::block(s, d);
    H::digest(out, s);
}

// "HPKE-v1" || "KEM" || BE16(kem id) at byte `off`: 12 bytes
CIRCL_HD void put_suite(uint32_t *m, int off, int kem_id) {
    put_bytes(m, off, "HPKE-v1");
    put_bytes(m, off + 7, "KEM");
    m[(off + 10) / 4] |= (uint32_t)((kem_id >> 8) & 0xff) << (8 * ((off + 10) % 4));
    m[(off + 11) / 4] |= (uint32_t)(kem_id & 0xff) << (8 * ((off + 11) % 4));
}

// kembase.go:52-61 labeledExtract with the empty salt: prk = HMAC(0, "HPKE-v1" || suite || label || ikm), ikm = IKM_WORDS words
template <class H, int KEM_ID, int IKM_WORDS, int LN>
CIRCL_HD void labeled_extract(uint32_t *prk, const char (&label)[LN], const uint32_t *ikm) {
    constexpr int LEN = 12 + (LN - 1) + 4 * IKM_WORDS, NW = msg_words<H>(LEN);
    uint32_t m[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) m[i] = 0;
    put_suite(m, 0, KEM_ID);
    put_bytes(m, 12, label);
#pragma unroll
    for (int i = 0; i < IKM_WORDS; i++) put_word(m, 12 + (LN - 1) + 4 * i, ikm[i]);
    hmac<H, LEN, true>(prk, nullptr, m);
}

// kembase.go:63-82 labeledExpand for L <= H::OUT bytes: the first L bytes of T(1) = HMAC(prk, BE16(L) || "HPKE-v1" || suite ||
// label || info || 01); info = INFO_WORDS words, out = L / 4 words
template <class H, int KEM_ID, int L, int INFO_WORDS, int LN>
CIRCL_HD void labeled_expand(uint32_t *out, const uint32_t *prk, const char (&label)[LN], const uint32_t *info) {
    static_assert(L > 0 && L <= H::OUT && L % 4 == 0, "one block of output");
    constexpr int LEN = 2 + 12 + (LN - 1) + 4 * INFO_WORDS + 1, NW = msg_words<H>(LEN);
    uint32_t m[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) m[i] = 0;
    m[0] = (uint32_t)((L >> 8) & 0xff) | ((uint32_t)(L & 0xff) << 8);
    put_suite(m, 2, KEM_ID);
    put_bytes(m, 14, label);
#pragma unroll
    for (int i = 0; i < INFO_WORDS; i++) put_word(m, 14 + (LN - 1) + 4 * i, info[i]);
    m[(LEN - 1) / 4] |= 1u << (8 * ((LEN - 1) % 4));
    uint32_t t[H::OUT / 4];
    hmac<H, LEN, false>(t, prk, m);
#pragma unroll
    for (int i = 0; i < L / 4; i++) out[i] = t[i];
}

}  // namespace hkdf
}  // namespace circl
