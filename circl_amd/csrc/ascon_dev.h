// ascon_dev.h -- the Ascon v1.2 AEADs Ascon128, Ascon128a and Ascon80pq (cipher/ascon/ascon.go), one item per lane.
//
// The state is five 64-bit words held as ten 32-bit registers (lo / hi), the key three words as in Cipher.key (word 0 has 32 bits).
// One round of the permutation on the tools of keccak_dev.h:
//     pC + pS : the three xors in front of chi (the round constant rides in the one of x2's low half as a third input), chi on five
//               words (bitop3_chi), the three xors behind it                                       = 11 three-input ops per half
//     pL      : x ^= ror(x, a) ^ ror(x, b): four alignbit and two three-input xors per word; the NOT that ends pS on x2 is the
//               truth table of x2's two xors here (~(p ^ q ^ r) is one op)                         = 30
// = 52 VALU instructions per round as written; round constants are template arguments.  What the compiler makes of it is recorded in
// DESIGN 4.8h and profiles/ascon_bench.txt.
//
// Bytes are big-endian inside a word.  Rows are byte-ragged and nothing past a row is read or written: plaintext, ciphertext and aad
// move byte by byte, the bytes of a partial block under predicates, as in chacha20poly1305_dev.h.  (Word loads with a byte swap for the
// full blocks of 4-byte aligned items were tried and did not beat this: profiles/ascon_bench.txt.)  Nothing branches on, or is indexed
// by, a key, the state or a plaintext: the loops run over the public lengths.  Open decrypts and authenticates in one pass: it writes
// the plaintext as it goes, ORs the tag's word differences, and zeroes its own plaintext row where the tag is wrong (the verdict is an
// output, so that branch is public).
#pragma once
#include <stdint.h>

#include <utility>

#include "keccak_dev.h"

namespace circl {
namespace ascon {

constexpr int ASCON128 = 1, ASCON128A = 2, ASCON80PQ = -1;  // ascon.go:54-58
constexpr int PERM_A = 12, TAG_BYTES = 16, NONCE_BYTES = 16;

constexpr bool mode_ok(int mode) { return mode == ASCON128 || mode == ASCON128A || mode == ASCON80PQ; }
constexpr int key_bytes(int mode) { return mode == ASCON80PQ ? 20 : mode_ok(mode) ? 16 : 0; }
constexpr int block_bytes(int mode) { return mode == ASCON128A ? 16 : 8; }  // ascon.go:170
constexpr int perm_b(int mode) { return mode == ASCON128A ? 8 : 6; }        // ascon.go:173

struct State {
    uint32_t lo[5], hi[5];
};
struct Key {  // Cipher.key: k0 < 2^32 (zero but for Ascon80pq)
    uint32_t k0, k1hi, k1lo, k2hi, k2lo;
};

CIRCL_HD uint32_t bitop3_xnor(uint32_t a, uint32_t b, uint32_t c) {  // ~(a ^ b ^ c)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x69);
#else
    return ~(a ^ b ^ c);
#endif
}
CIRCL_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

template <int R>
CIRCL_HD void ror64(uint32_t &olo, uint32_t &ohi, uint32_t lo, uint32_t hi) {
    static_assert(R > 0 && R < 64 && R != 32, "a rotation that two funnel shifts make");
    if constexpr (R < 32) {
        olo = alignbit(hi, lo, R); ohi = alignbit(lo, hi, R);
    } else {
        olo = alignbit(lo, hi, R - 32); ohi = alignbit(hi, lo, R - 32);
    }
}
// x ^= ror(x, A) ^ ror(x, B) on a (lo, hi) pair, complemented with NOT
template <int A, int B, bool NOT = false>
CIRCL_HD void diffuse(uint32_t &lo, uint32_t &hi) {
    uint32_t al, ah, bl, bh;
    ror64<A>(al, ah, lo, hi);
    ror64<B>(bl, bh, lo, hi);
    lo = NOT ? bitop3_xnor(lo, al, bl) : bitop3_xor(lo, al, bl);
    hi = NOT ? bitop3_xnor(hi, ah, bh) : bitop3_xor(hi, ah, bh);
}

// pC and pS (ascon.go:264-285 without the final NOT of x2, which diffuse<.., true> applies) on one half of the five words
template <uint32_t C>
CIRCL_HD void sbox(uint32_t *x) {
    const uint32_t a0 = x[0] ^ x[4], a1 = x[1], a2 = C ? bitop3_xor(x[2], x[1], C) : x[2] ^ x[1], a3 = x[3], a4 = x[4] ^ x[3];
    const uint32_t b0 = bitop3_chi(a0, a1, a2), b1 = bitop3_chi(a1, a2, a3), b2 = bitop3_chi(a2, a3, a4), b3 = bitop3_chi(a3, a4, a0),
                   b4 = bitop3_chi(a4, a0, a1);
    x[0] = b0 ^ b4; x[1] = b1 ^ b0; x[2] = b2; x[3] = b3 ^ b2; x[4] = b4;
}

template <int I>  // round I of 12
CIRCL_HD void round(State &s) {
    sbox<uint32_t((0xF - I) << 4 | I)>(s.lo);
    sbox<0>(s.hi);
    diffuse<19, 28>(s.lo[0], s.hi[0]);
    diffuse<61, 39>(s.lo[1], s.hi[1]);
    diffuse<1, 6, true>(s.lo[2], s.hi[2]);
    diffuse<10, 17>(s.lo[3], s.hi[3]);
    diffuse<7, 41>(s.lo[4], s.hi[4]);
}
template <int ROUNDS, int... I>
CIRCL_HD void perm_rounds(State &s, std::integer_sequence<int, I...>) {
    (round<PERM_A - ROUNDS + I>(s), ...);
}
// ascon.go:260-295 perm(ROUNDS, s): the last ROUNDS of the twelve rounds
template <int ROUNDS>
CIRCL_HD void perm(State &s) {
    static_assert(ROUNDS >= 1 && ROUNDS <= PERM_A, "");
    perm_rounds<ROUNDS>(s, std::make_integer_sequence<int, ROUNDS>());
}

// ---- bytes <-> big-endian words ---------------------------------------------------------------------------------------------------
// the 8 bytes p[0 .. 8) as (hi, lo)
CIRCL_HD void load_block(uint32_t &hi, uint32_t &lo, const uint8_t *p) {
    hi = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    lo = (uint32_t)p[4] << 24 | (uint32_t)p[5] << 16 | (uint32_t)p[6] << 8 | p[7];
}
CIRCL_HD void store_block(uint8_t *p, uint32_t hi, uint32_t lo) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        p[k] = (uint8_t)(hi >> (24 - 8 * k));
        p[4 + k] = (uint8_t)(lo >> (24 - 8 * k));
    }
}
// the nb <= 8 bytes p[at .. at + nb) as (hi, lo), zeros behind them (p may be NULL where nb == 0: no address is formed)
CIRCL_HD void load_partial(uint32_t &hi, uint32_t &lo, const uint8_t *p, int at, uint32_t nb) {
    hi = lo = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((uint32_t)k < nb) hi |= (uint32_t)p[at + k] << (24 - 8 * k);
        if ((uint32_t)k + 4 < nb) lo |= (uint32_t)p[at + 4 + k] << (24 - 8 * k);
    }
}
CIRCL_HD void store_partial(uint8_t *p, int at, uint32_t hi, uint32_t lo, uint32_t nb) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((uint32_t)k < nb) p[at + k] = (uint8_t)(hi >> (24 - 8 * k));
        if ((uint32_t)k + 4 < nb) p[at + 4 + k] = (uint8_t)(lo >> (24 - 8 * k));
    }
}
// ones over the first nb <= 8 bytes of a word, and the byte v at byte position k < 8
CIRCL_HD void head_mask(uint32_t &hi, uint32_t &lo, uint32_t nb) {
    hi = nb >= 4 ? 0xffffffffu : nb ? 0xffffffffu << (32 - 8 * nb) : 0u;
    lo = nb >= 8 ? 0xffffffffu : nb > 4 ? 0xffffffffu << (64 - 8 * nb) : 0u;
}
CIRCL_HD void byte_at(uint32_t &hi, uint32_t &lo, uint32_t k, uint32_t v) {
    hi = k < 4 ? v << (24 - 8 * k) : 0u;
    lo = k < 4 ? 0u : v << (56 - 8 * k);
}
// how many of the bytes [8 w, 8 w + 8) lie below len
CIRCL_HD uint32_t bytes_in_word(uint64_t len, int w) { return len <= 8u * w ? 0u : len - 8u * w >= 8 ? 8u : (uint32_t)(len - 8u * w); }

// ---- the cipher (ascon.go:70-93, 175-258) -----------------------------------------------------------------------------------------
// key: the row as KeySize / 4 words the way memory holds them
template <int MODE>
CIRCL_HD void load_key(Key &k, const uint32_t *key) {
    if constexpr (MODE == ASCON80PQ) {
        k.k0 = bswap32(key[0]);
        k.k1hi = bswap32(key[1]); k.k1lo = bswap32(key[2]); k.k2hi = bswap32(key[3]); k.k2lo = bswap32(key[4]);
    } else {
        k.k0 = 0;
        k.k1hi = bswap32(key[0]); k.k1lo = bswap32(key[1]); k.k2hi = bswap32(key[2]); k.k2lo = bswap32(key[3]);
    }
}

template <int MODE>
CIRCL_HD void initialize(State &s, const Key &k, const uint32_t *nonce) {
    s.hi[0] = (uint32_t)key_bytes(MODE) * 8u << 24 | (uint32_t)block_bytes(MODE) * 8u << 16 | (uint32_t)PERM_A << 8 | (uint32_t)perm_b(MODE);
    s.lo[0] = k.k0;
    s.hi[1] = k.k1hi; s.lo[1] = k.k1lo;
    s.hi[2] = k.k2hi; s.lo[2] = k.k2lo;
    s.hi[3] = bswap32(nonce[0]); s.lo[3] = bswap32(nonce[1]);
    s.hi[4] = bswap32(nonce[2]); s.lo[4] = bswap32(nonce[3]);
    perm<PERM_A>(s);
    s.lo[2] ^= k.k0;
    s.hi[3] ^= k.k1hi; s.lo[3] ^= k.k1lo;
    s.hi[4] ^= k.k2hi; s.lo[4] ^= k.k2lo;
}

// The text's last, partial block (len < the block size, possibly 0) and the padding bit behind it: absorbed (ABSORB: s ^= in, nothing is
// written), encrypted (ENC: out = s ^ in becomes the state) or decrypted (out = s ^ in, the input's bytes become the state's).
template <int MODE, bool ABSORB, bool ENC>
CIRCL_HD void last_block(State &s, uint8_t *out, const uint8_t *in, uint64_t len) {
#pragma unroll
    for (int w = 0; w < block_bytes(MODE) / 8; w++) {
        const uint32_t nb = bytes_in_word(len, w);
        uint32_t ih, il, ph = 0, pl = 0;
        load_partial(ih, il, in, 8 * w, nb);
        if (!ABSORB) store_partial(out, 8 * w, s.hi[w] ^ ih, s.lo[w] ^ il, nb);
        if (len >= 8u * w && len < 8u * w + 8) byte_at(ph, pl, (uint32_t)(len - 8u * w), 0x80u);
        if (ABSORB || ENC) {
            s.hi[w] = bitop3_xor(s.hi[w], ih, ph); s.lo[w] = bitop3_xor(s.lo[w], il, pl);
        } else {
            uint32_t mh, ml;
            head_mask(mh, ml, nb);
            s.hi[w] = ((s.hi[w] & ~mh) | ih) ^ ph; s.lo[w] = ((s.lo[w] & ~ml) | il) ^ pl;
        }
    }
}

template <int MODE>
CIRCL_HD void assoc_data(State &s, const uint8_t *add, uint64_t len) {
    constexpr int BS = block_bytes(MODE);
    if (len > 0) {
        for (; len >= BS; add += BS, len -= BS) {
#pragma unroll
            for (int w = 0; w < BS / 8; w++) {
                uint32_t ih, il;
                load_block(ih, il, add + 8 * w);
                s.hi[w] ^= ih; s.lo[w] ^= il;
            }
            perm<perm_b(MODE)>(s);
        }
        last_block<MODE, true, true>(s, nullptr, add, len);
        perm<perm_b(MODE)>(s);
    }
    s.lo[4] ^= 1u;
}

// ascon.go:212-242 for Seal (ENC) and Open
template <int MODE, bool ENC>
CIRCL_HD void proc_text(State &s, uint8_t *out, const uint8_t *in, uint64_t len) {
    constexpr int BS = block_bytes(MODE);
    for (; len >= BS; in += BS, out += BS, len -= BS) {
#pragma unroll
        for (int w = 0; w < BS / 8; w++) {
            uint32_t ih, il;
            load_block(ih, il, in + 8 * w);
            const uint32_t oh = s.hi[w] ^ ih, ol = s.lo[w] ^ il;
            store_block(out + 8 * w, oh, ol);
            s.hi[w] = ENC ? oh : ih; s.lo[w] = ENC ? ol : il;
        }
        perm<perm_b(MODE)>(s);
    }
    last_block<MODE, false, ENC>(s, out, in, len);
}

// ascon.go:244-258: the tag as (s3 ^ k1, s4 ^ k2)
template <int MODE>
CIRCL_HD void finalize(State &s, const Key &k, uint32_t *tag) {
    constexpr int W = block_bytes(MODE) / 8;
    if constexpr (MODE == ASCON80PQ) {
        s.hi[W] ^= k.k0; s.lo[W] ^= k.k1hi;
        s.hi[W + 1] ^= k.k1lo; s.lo[W + 1] ^= k.k2hi;
        s.hi[W + 2] ^= k.k2lo;
    } else {
        s.hi[W] ^= k.k1hi; s.lo[W] ^= k.k1lo;
        s.hi[W + 1] ^= k.k2hi; s.lo[W + 1] ^= k.k2lo;
    }
    perm<PERM_A>(s);
    tag[0] = s.hi[3] ^ k.k1hi; tag[1] = s.lo[3] ^ k.k1lo;
    tag[2] = s.hi[4] ^ k.k2hi; tag[3] = s.lo[4] ^ k.k2lo;
}

// Cipher.Seal: ct[0 .. pt_len + 16) = ct || tag
template <int MODE>
CIRCL_HD void seal(uint8_t *ct, const uint32_t *key, const uint32_t *nonce, const uint8_t *pt, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len) {
    Key k;
    State s;
    uint32_t tag[4];
    load_key<MODE>(k, key);
    initialize<MODE>(s, k, nonce);
    assoc_data<MODE>(s, aad, aad_len);
    proc_text<MODE, true>(s, ct, pt, pt_len);
    finalize<MODE>(s, k, tag);
    store_block(ct + pt_len, tag[0], tag[1]);
    store_block(ct + pt_len + 8, tag[2], tag[3]);
}

// Cipher.Open: pt[0 .. pt_len) from ct[0 .. pt_len + 16); returns 1, or 0 with an all-zero pt (the reference's clear(plaintext))
template <int MODE>
CIRCL_HD uint32_t open(uint8_t *pt, const uint32_t *key, const uint32_t *nonce, const uint8_t *ct, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len) {
    Key k;
    State s;
    uint32_t tag[4], got[4];
    load_key<MODE>(k, key);
    initialize<MODE>(s, k, nonce);
    assoc_data<MODE>(s, aad, aad_len);
    proc_text<MODE, false>(s, pt, ct, pt_len);
    finalize<MODE>(s, k, tag);
    load_block(got[0], got[1], ct + pt_len);
    load_block(got[2], got[3], ct + pt_len + 8);
    const uint32_t diff = (tag[0] ^ got[0]) | (tag[1] ^ got[1]) | (tag[2] ^ got[2]) | (tag[3] ^ got[3]);
    const uint32_t good = 1u ^ ((diff | (0u - diff)) >> 31);
    if (!good) {  // (public: ok is an output)
        for (uint64_t o = 0; o < pt_len; o++) pt[o] = 0;
    }
    return good;
}

}  // namespace ascon
}  // namespace circl
