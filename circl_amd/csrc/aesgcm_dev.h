// aesgcm_dev.h -- AES-128-GCM and AES-256-GCM (NIST SP 800-38D over FIPS 197; hpke/aead.go through crypto/aes and crypto/cipher), one
// item per lane, 12-byte nonces and 16-byte tags.  CDNA has neither an AES round nor a carry-less multiply, so both halves are
// constant-time software: nothing here loads from an address, or branches on a value, that depends on a key, a plaintext, H or a tag.
// There is no S-box table, no T-table and no table of multiples of H.  Lengths, offsets, the key size and Open's verdict are public.
//
// AES, encryption only (CTR and GHASH never decrypt a block), bitsliced inside the lane: eight 32-bit words hold two blocks, word b
// = bit b of all 32 bytes, the byte of row r and column c of block k at bit 8 r + 2 c + k.  In that layout
//     SubBytes    is the 113-gate circuit of Boyar and Peralta (eprint 2009/191: 32 AND, 77 XOR, 4 XNOR) on the eight words,
//     ShiftRows   rotates byte r of every word by 2 r bits (two byte-wise rotations under byte masks),
//     MixColumns  is x ^ rotr8(x) per word, one neighbour word for the doubling (and word 7 for the reduction by 0x1B), rotr16,
//     AddRoundKey widens the round key, see below.
// ortho() is the 8 x 8 bit transpose between four little-endian words per block and the eight bit planes (12 masked swaps).  A pass
// encrypts two blocks: the two counter blocks of 32 bytes of text, or, as every item's first pass, 0^128 and J0, which gives H and
// E_K(J0) together.  The pass has ONE call site (the loop in crypt()), so its unrolled rounds exist once per kernel.
//
// Round keys are per item.  Both blocks of a pass take the same key, so the bit planes of a round key carry each bit twice (k = 0 and
// k = 1): the schedule keeps only the 16 distinct bits per plane, two planes to a word -- 4 words per round key, 44 (AES-128) or 60
// (AES-256) in all -- in VGPRs, and AddRoundKey widens a word to its two planes with four operations.  The rounds are unrolled, so
// every index into that array is a constant and it never leaves the register file (DESIGN 4.8i has what the compiler reports and
// why LDS, scratch and a schedule per pass were not built).  The schedule's SubWord runs the same circuit on four bytes.  A key
// shared by the batch is expanded per lane, by the same code: all 64 lanes of a wavefront execute the schedule whether one of them
// needs it or all do, so once per wavefront saves nothing unless the round keys move to SGPRs, which is another kernel.
//
// GHASH: Y <- (Y ^ X) * H in GF(2^128) with GCM's bit order (bit 0 of a block is the coefficient of x^0 and the top bit of byte 0),
// blocks held as four big-endian words.  The product is masked shift-and-xor, four bits of Y a step: for j = 0 .. 31, the bit j of
// each of Y's four words (as an all-ones / all-zero mask, made by arithmetic) gates V_j = H x^j into one of four accumulators, and
// V_{j+1} = V_j x is a 128-bit shift right by one and a masked xor of 0xE1 << 24.  The accumulators meet by Horner's rule in x^32:
// times x^32 moves words and folds the word that falls off with x^128 = x^7 + x^2 + x + 1.
//
// Seal writes ct || tag.  Open authenticates the whole ciphertext first and then decrypts under the verdict as a mask: a failed item
// has an all-zero plaintext row, and no unauthenticated plaintext byte reaches memory.  Rows are byte-ragged and nothing past a row
// is read or written: text and aad move byte by byte under predicates (chacha20poly1305_dev.h load_chunk / store_chunk).  Argument
// order and meaning of seal / open are those of chapoly::seal / chapoly::open: the key and the nonce as words the way memory holds
// them.  Distinct (key, nonce) pairs are the caller's duty, as with Go's cipher.AEAD.
#pragma once
#include <stdint.h>

#include "chacha20poly1305_dev.h"
#include "keccak_dev.h"

namespace circl {
namespace aesgcm {

constexpr int AES128GCM = 16, AES256GCM = 32;   // = the key size in bytes
constexpr int TAG_BYTES = 16, NONCE_BYTES = 12;
constexpr uint64_t MAX_PT_BYTES = (uint64_t(1) << 36) - 32;   // SP 800-38D 5.2.1.1: 2^39 - 256 bits

constexpr bool key_bytes_ok(int kb) { return kb == AES128GCM || kb == AES256GCM; }
constexpr int rounds(int kb) { return kb / 4 + 6; }
constexpr int rk_words(int kb) { return 4 * (rounds(kb) + 1); }   // FIPS 197's w[], and as many compact words

CIRCL_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
CIRCL_HD uint32_t rotr(uint32_t v, uint32_t s) { return alignbit(v, v, s); }

// the round keys in compact form: word 4 r + u = the planes 2 u (even bits) and 2 u + 1 (odd bits) of round key r
template <int KB>
struct RoundKeys {
    uint32_t c[rk_words(KB)];
};

// ---- the bit planes ----------------------------------------------------------------------------------------------------------------
// q[0 .. 8) <-> its 8 x 8 bit transpose: bit 8 k + i of word j <-> bit 8 k + j of word i.  An involution.
CIRCL_HD void swap_bits(uint32_t &x, uint32_t &y, uint32_t lo, int s) {
    const uint32_t a = x, b = y;
    x = (a & lo) | ((b & lo) << s);
    y = ((a & ~lo) >> s) | (b & ~lo);
}
CIRCL_HD void ortho(uint32_t *q) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) swap_bits(q[i], q[i + 1], 0x55555555u, 1);
#pragma unroll
    for (int i = 0; i < 8; i += 4) {
        swap_bits(q[i], q[i + 2], 0x33333333u, 2);
        swap_bits(q[i + 1], q[i + 3], 0x33333333u, 2);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) swap_bits(q[i], q[i + 4], 0x0F0F0F0Fu, 4);
}

// SubBytes on eight bit planes (q[b] = bit b of every byte): Boyar and Peralta's circuit, whose x0 / s0 are the top bits
CIRCL_HD void sbox(uint32_t *q) {
    const uint32_t x0 = q[7], x1 = q[6], x2 = q[5], x3 = q[4], x4 = q[3], x5 = q[2], x6 = q[1], x7 = q[0];
    // the top linear layer
    const uint32_t y14 = x3 ^ x5, y13 = x0 ^ x6, y9 = x0 ^ x3, y8 = x0 ^ x5, t0 = x1 ^ x2, y1 = t0 ^ x7, y4 = y1 ^ x3, y12 = y13 ^ y14;
    const uint32_t y2 = y1 ^ x0, y5 = y1 ^ x6, y3 = y5 ^ y8, t1 = x4 ^ y12, y15 = t1 ^ x5, y20 = t1 ^ x1, y6 = y15 ^ x7, y10 = y15 ^ t0;
    const uint32_t y11 = y20 ^ y9, y7 = x7 ^ y11, y17 = y10 ^ y11, y19 = y10 ^ y8, y16 = t0 ^ y11, y21 = y13 ^ y16, y18 = x0 ^ y16;
    // the inversion in GF(2^8) over GF(2^4) over GF(2^2)
    const uint32_t t2 = y12 & y15, t3 = y3 & y6, t4 = t3 ^ t2, t5 = y4 & x7, t6 = t5 ^ t2, t7 = y13 & y16, t8 = y5 & y1, t9 = t8 ^ t7;
    const uint32_t t10 = y2 & y7, t11 = t10 ^ t7, t12 = y9 & y11, t13 = y14 & y17, t14 = t13 ^ t12, t15 = y8 & y10, t16 = t15 ^ t12;
    const uint32_t t17 = t4 ^ t14, t18 = t6 ^ t16, t19 = t9 ^ t14, t20 = t11 ^ t16, t21 = t17 ^ y20, t22 = t18 ^ y19, t23 = t19 ^ y21, t24 = t20 ^ y18;
    const uint32_t t25 = t21 ^ t22, t26 = t21 & t23, t27 = t24 ^ t26, t28 = t25 & t27, t29 = t28 ^ t22, t30 = t23 ^ t24, t31 = t22 ^ t26;
    const uint32_t t32 = t31 & t30, t33 = t32 ^ t24, t34 = t23 ^ t33, t35 = t27 ^ t33, t36 = t24 & t35, t37 = t36 ^ t34, t38 = t27 ^ t36;
    const uint32_t t39 = t29 & t38, t40 = t25 ^ t39;
    const uint32_t t41 = t40 ^ t37, t42 = t29 ^ t33, t43 = t29 ^ t40, t44 = t33 ^ t37, t45 = t42 ^ t41;
    const uint32_t z0 = t44 & y15, z1 = t37 & y6, z2 = t33 & x7, z3 = t43 & y16, z4 = t40 & y1, z5 = t29 & y7, z6 = t42 & y11, z7 = t45 & y17;
    const uint32_t z8 = t41 & y10, z9 = t44 & y12, z10 = t37 & y3, z11 = t33 & y4, z12 = t43 & y13, z13 = t40 & y5, z14 = t29 & y2, z15 = t42 & y9;
    const uint32_t z16 = t45 & y14, z17 = t41 & y8;
    // the bottom linear layer
    const uint32_t t46 = z15 ^ z16, t47 = z10 ^ z11, t48 = z5 ^ z13, t49 = z9 ^ z10, t50 = z2 ^ z12, t51 = z2 ^ z5, t52 = z7 ^ z8, t53 = z0 ^ z3;
    const uint32_t t54 = z6 ^ z7, t55 = z16 ^ z17, t56 = z12 ^ t48, t57 = t50 ^ t53, t58 = z4 ^ t46, t59 = z3 ^ t54, t60 = t46 ^ t57, t61 = z14 ^ t57;
    const uint32_t t62 = t52 ^ t58, t63 = t49 ^ t58, t64 = z4 ^ t59, t65 = t61 ^ t62, t66 = z1 ^ t63;
    const uint32_t s0 = t59 ^ t63, s6 = ~(t56 ^ t62), s7 = ~(t48 ^ t60), t67 = t64 ^ t65, s3 = t53 ^ t66, s4 = t51 ^ t66, s5 = t47 ^ t65;
    const uint32_t s1 = ~(t64 ^ s3), s2 = ~(t55 ^ t67);
    q[7] = s0; q[6] = s1; q[5] = s2; q[4] = s3; q[3] = s4; q[2] = s5; q[1] = s6; q[0] = s7;
}

// the bits of byte r of every plane are 2 c + k: row r moves left by r columns = byte r rotates right by 2 r bits
CIRCL_HD uint32_t shift_rows_word(uint32_t x) {
    const uint32_t r2 = ((x >> 2) & 0x3F3F3F3Fu) | ((x << 6) & 0xC0C0C0C0u);    // every byte by 2: taken by rows 1 and 3
    x = (x & 0x00FF00FFu) | (r2 & 0xFF00FF00u);
    const uint32_t r4 = ((x >> 4) & 0x0F0F0F0Fu) | ((x << 4) & 0xF0F0F0F0u);    // every byte by 4: taken by rows 2 and 3
    return (x & 0x0000FFFFu) | (r4 & 0xFFFF0000u);
}

// row r + 1 of a column is the next byte of the word: out = 2 (a ^ a') ^ a' ^ (a'' ^ a'''), the doubling one plane up
CIRCL_HD void mix_columns(uint32_t *q) {
    uint32_t r[8], t[8];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        r[b] = rotr(q[b], 8);
        t[b] = q[b] ^ r[b];
    }
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const uint32_t far = rotr(t[b], 16);
        if (b == 0) q[b] = bitop3_xor(t[7], r[b], far);
        else if (b == 1 || b == 3 || b == 4) q[b] = bitop3_xor(t[b - 1], r[b], far) ^ t[7];   // 0x1B: planes 0, 1, 3, 4
        else q[b] = bitop3_xor(t[b - 1], r[b], far);
    }
}

// The widened planes do not change from pass to pass, so the compiler would hoist all 88 / 120 of them out of the pass loop and
// spill them (237 - 271 VGPR spills were reported that way); the empty asm makes the compact word opaque at its use.
template <int KB>
CIRCL_HD void add_round_key(uint32_t *q, const RoundKeys<KB> &rk, int r) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        uint32_t c = rk.c[4 * r + u];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(c));
#endif
        const uint32_t even = c & 0x55555555u, odd = c & 0xAAAAAAAAu;
        q[2 * u] ^= even | (even << 1);
        q[2 * u + 1] ^= odd | (odd >> 1);
    }
}

// SubWord of FIPS 197 5.2 on one little-endian word: the planes of four bytes sit at bits 0, 8, 16, 24 (the other bits compute S(0))
CIRCL_HD uint32_t sub_word(uint32_t w) {
    uint32_t q[8], out = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) q[b] = (w >> b) & 0x01010101u;
    sbox(q);
#pragma unroll
    for (int b = 0; b < 8; b++) out |= (q[b] & 0x01010101u) << b;
    return out;
}

constexpr uint32_t rcon(int i) { return i < 8 ? 1u << i : i == 8 ? 0x1Bu : 0x36u; }

// FIPS 197 5.2; key: the row as KB / 4 words the way memory holds them (a column of the state is one little-endian word)
template <int KB>
CIRCL_HD void expand_key(RoundKeys<KB> &rk, const uint32_t *key) {
    constexpr int NK = KB / 4, NW = rk_words(KB);
    uint32_t w[NW];
    detail::static_for<0, NW>([&](auto ic) {
        constexpr int i = decltype(ic)::v;
        if constexpr (i < NK) {
            w[i] = key[i];
        } else {
            uint32_t t = w[i - 1];
            if constexpr (i % NK == 0) t = sub_word(rotr(t, 8)) ^ rcon(i / NK - 1);
            else if constexpr (NK > 6 && i % NK == 4) t = sub_word(t);
            w[i] = w[i - NK] ^ t;
        }
        if constexpr (i % 4 == 3) {   // a round key is complete: to its compact planes at once, so that w[] is live NK words back only
            constexpr int r = i / 4;
            uint32_t q[8];
#pragma unroll
            for (int c = 0; c < 4; c++) q[2 * c] = q[2 * c + 1] = w[4 * r + c];
            ortho(q);
#pragma unroll
            for (int u = 0; u < 4; u++) rk.c[4 * r + u] = (q[2 * u] & 0x55555555u) | (q[2 * u + 1] & 0xAAAAAAAAu);
        }
    });
}

// FIPS 197 5.1 on two blocks: q[2 c + k] = column c of block k as a little-endian word, in and out
template <int KB>
CIRCL_HD void encrypt2(uint32_t *q, const RoundKeys<KB> &rk) {
    constexpr int NR = rounds(KB);
    ortho(q);
    add_round_key<KB>(q, rk, 0);
    detail::static_for<1, NR>([&](auto ic) {
        sbox(q);
#pragma unroll
        for (int b = 0; b < 8; b++) q[b] = shift_rows_word(q[b]);
        mix_columns(q);
        add_round_key<KB>(q, rk, decltype(ic)::v);
    });
    sbox(q);
#pragma unroll
    for (int b = 0; b < 8; b++) q[b] = shift_rows_word(q[b]);
    add_round_key<KB>(q, rk, NR);
    ortho(q);
}

// ---- GHASH (SP 800-38D 6.3, 6.4): blocks as four big-endian words, word 0 first ---------------------------------------------------
// z <- z x^32: the word that falls off is x^128 .. x^159 = (x^7 + x^2 + x + 1) x^0 .. x^31, which reaches into word 1 and no further
CIRCL_HD void ghash_mulx32(uint32_t *z) {
    const uint32_t t = z[3];
    z[3] = z[2];
    z[2] = z[1];
    z[1] = z[0] ^ bitop3_xor(t << 31, t << 30, t << 25);
    z[0] = t ^ bitop3_xor(t >> 1, t >> 2, t >> 7);
}

// y <- y * h
CIRCL_HD void ghash_mul(uint32_t *y, const uint32_t *h) {
    uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
    uint32_t a[4][4] = {};
#pragma nounroll
    for (int j = 0; j < 32; j++) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t m = (uint32_t)((int32_t)(y[w] << j) >> 31);   // the coefficient of x^(32 w + j), all ones or zero
            a[w][0] = bitop3_xor_and(a[w][0], v0, m);
            a[w][1] = bitop3_xor_and(a[w][1], v1, m);
            a[w][2] = bitop3_xor_and(a[w][2], v2, m);
            a[w][3] = bitop3_xor_and(a[w][3], v3, m);
        }
        const uint32_t carry = 0u - (v3 & 1u);
        v3 = alignbit(v2, v3, 1);
        v2 = alignbit(v1, v2, 1);
        v1 = alignbit(v0, v1, 1);
        v0 = bitop3_xor_and(v0 >> 1, carry, 0xE1000000u);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) y[k] = a[3][k];
#pragma unroll
    for (int w = 2; w >= 0; w--) {
        ghash_mulx32(y);
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] ^= a[w][k];
    }
}

// one block of four little-endian words (the way text is loaded and AES speaks) into the hash
CIRCL_HD void ghash_block(uint32_t *y, const uint32_t *h, const uint32_t *le) {
#pragma unroll
    for (int k = 0; k < 4; k++) y[k] ^= bswap32(le[k]);
    ghash_mul(y, h);
}
// the range p[0 .. len), zero-padded to a multiple of 16 (p may be NULL where len == 0: no address is formed)
CIRCL_HD void ghash_padded(uint32_t *y, const uint32_t *h, const uint8_t *p, uint64_t len) {
    for (uint64_t o = 0; o < len; o += 16) {
        uint32_t w[4];
        chapoly::load_chunk(w, p + o, len - o < 16 ? (uint32_t)(len - o) : 16u);
        ghash_block(y, h, w);
    }
}
CIRCL_HD void ghash_lengths(uint32_t *y, const uint32_t *h, uint64_t aad_len, uint64_t ct_len) {
    y[0] ^= (uint32_t)(aad_len >> 29); y[1] ^= (uint32_t)(aad_len << 3);
    y[2] ^= (uint32_t)(ct_len >> 29); y[3] ^= (uint32_t)(ct_len << 3);
    ghash_mul(y, h);
}

// ---- the AEAD ----------------------------------------------------------------------------------------------------------------------
// Both directions are one loop over passes of two blocks, so that encrypt2 is instantiated once.  Pass 0 encrypts 0^128 and J0 =
// nonce || 1 and hashes what is known by then: the aad for Seal; aad, ciphertext and lengths for Open, whose verdict becomes the
// mask of every later store.  Pass p > 0 makes the keystream of counters 2 p and 2 p + 1 (inc32: the counter is a 32-bit big-endian
// word) for the bytes [32 (p - 1), 32 p).  `gate`: Seal's mask (all ones, or 0 for an item that failed before: an all-zero row), or
// Open's verdict so far (0 or 1).  Returns Open's verdict.
template <int KB, bool SEAL>
CIRCL_HD uint32_t crypt(uint8_t *out, const uint32_t *key, const uint32_t *nonce, const uint8_t *in, uint64_t len, const uint8_t *aad, uint64_t aad_len,
                        uint32_t gate) {
    RoundKeys<KB> rk;
    expand_key<KB>(rk, key);
    uint32_t h[4] = {}, y[4] = {}, ej0[4] = {}, tag[4];
    uint32_t mask = SEAL ? gate : 0u, good = gate;
    for (uint64_t p = 0; p == 0 || 32 * (p - 1) < len; p++) {
        uint32_t q[8];
        q[0] = p ? nonce[0] : 0u; q[2] = p ? nonce[1] : 0u; q[4] = p ? nonce[2] : 0u; q[6] = p ? bswap32((uint32_t)(2 * p)) : 0u;
        q[1] = nonce[0]; q[3] = nonce[1]; q[5] = nonce[2]; q[7] = bswap32((uint32_t)(2 * p + 1));
        encrypt2<KB>(q, rk);
        if (p == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                h[k] = bswap32(q[2 * k]);
                ej0[k] = q[2 * k + 1];
            }
            ghash_padded(y, h, aad, aad_len);
            if (!SEAL) {
                uint32_t got[4];
                ghash_padded(y, h, in, len);
                ghash_lengths(y, h, aad_len, len);
                chapoly::load_chunk(got, in + len, 16);
                uint32_t diff = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) diff |= (bswap32(y[k]) ^ ej0[k]) ^ got[k];
                good &= 1u ^ ((diff | (0u - diff)) >> 31);
                mask = 0u - good;
            }
        } else {
#pragma unroll
            for (int blk = 0; blk < 2; blk++) {
                const uint64_t at = 32 * (p - 1) + 16 * blk;
                if (at < len) {
                    const uint32_t nb = len - at < 16 ? (uint32_t)(len - at) : 16u;
                    uint32_t w[4];
                    chapoly::load_chunk(w, in + at, nb);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t keep = nb >= 4u * k + 4 ? 0xffffffffu : nb > 4u * k ? (1u << (8 * (nb - 4u * k))) - 1u : 0u;
                        w[k] = (w[k] ^ q[2 * k + blk]) & keep;
                    }
                    if (SEAL) ghash_block(y, h, w);
#pragma unroll
                    for (int k = 0; k < 4; k++) w[k] &= mask;
                    chapoly::store_chunk(out + at, w, nb);
                }
            }
        }
    }
    if (SEAL) {
        ghash_lengths(y, h, aad_len, len);
#pragma unroll
        for (int k = 0; k < 4; k++) tag[k] = (bswap32(y[k]) ^ ej0[k]) & mask;
        chapoly::store_chunk(out + len, tag, 16);
    }
    return good;
}

// ct[0 .. pt_len + 16) = Seal(key, nonce, pt, aad), every byte ANDed with mask (all ones, or 0 for an item that failed before)
template <int KB>
CIRCL_HD void seal(uint8_t *ct, const uint32_t *key, const uint32_t *nonce, const uint8_t *pt, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len,
                   uint32_t mask) {
    crypt<KB, true>(ct, key, nonce, pt, pt_len, aad, aad_len, mask);
}

// pt[0 .. pt_len) = Open(key, nonce, ct[0 .. pt_len + 16), aad); returns 1, or 0 with an all-zero pt.  `good` = the item's verdict
// so far (0 or 1): a 0 gives 0.
template <int KB>
CIRCL_HD uint32_t open(uint8_t *pt, const uint32_t *key, const uint32_t *nonce, const uint8_t *ct, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len,
                       uint32_t good) {
    return crypt<KB, false>(pt, key, nonce, ct, pt_len, aad, aad_len, good);
}

}  // namespace aesgcm
}  // namespace circl
