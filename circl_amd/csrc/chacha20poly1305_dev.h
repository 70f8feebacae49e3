// chacha20poly1305_dev.h -- the ChaCha20-Poly1305 AEAD (RFC 8439; hpke/aead.go through golang.org/x/crypto/chacha20poly1305), one
// item per lane.
//
// ChaCha20: the 16-word state in registers, 10 double rounds of add / rotate / xor.  Poly1305: the accumulator and r as five
// 26-bit limbs, a block is 25 32 x 32 -> 64-bit products, the final reduction is complete (h may be >= p before it) and the tag
// compare is a difference ORed over the four words.  Nothing branches on, or is indexed by, a secret: the loops run over the
// public lengths, and the bytes of a partial chunk are picked with predicated loads and stores.
//
// Seal writes ct || tag.  Open computes the tag over the ciphertext first and then decrypts under the verdict as a mask: a
// failed item's plaintext row is all zero.  Plaintext and ciphertext are read and written byte by byte (rows are byte-ragged and
// nothing past a row is touched).
#pragma once
#include <stdint.h>

#include "hkdf_dev.h"

namespace circl {
namespace chapoly {

CIRCL_HD uint32_t rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define CIRCL_CHACHA_QR(a, b, c, d) \
    a += b; d = rotl(d ^ a, 16);    \
    c += d; b = rotl(b ^ c, 12);    \
    a += b; d = rotl(d ^ a, 8);     \
    c += d; b = rotl(b ^ c, 7)

// RFC 8439 2.3: out = the 64-byte block of (key, counter, nonce) as 16 little-endian words
CIRCL_HD void chacha20_block(uint32_t *out, const uint32_t *key, uint32_t counter, const uint32_t *nonce) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                             key[4], key[5], key[6], key[7], counter, nonce[0], nonce[1], nonce[2]};
    uint32_t x0 = in[0], x1 = in[1], x2 = in[2], x3 = in[3], x4 = in[4], x5 = in[5], x6 = in[6], x7 = in[7];
    uint32_t x8 = in[8], x9 = in[9], x10 = in[10], x11 = in[11], x12 = in[12], x13 = in[13], x14 = in[14], x15 = in[15];
    for (int i = 0; i < 10; i++) {
        CIRCL_CHACHA_QR(x0, x4, x8, x12);
        CIRCL_CHACHA_QR(x1, x5, x9, x13);
        CIRCL_CHACHA_QR(x2, x6, x10, x14);
        CIRCL_CHACHA_QR(x3, x7, x11, x15);
        CIRCL_CHACHA_QR(x0, x5, x10, x15);
        CIRCL_CHACHA_QR(x1, x6, x11, x12);
        CIRCL_CHACHA_QR(x2, x7, x8, x13);
        CIRCL_CHACHA_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + in[0]; out[1] = x1 + in[1]; out[2] = x2 + in[2]; out[3] = x3 + in[3];
    out[4] = x4 + in[4]; out[5] = x5 + in[5]; out[6] = x6 + in[6]; out[7] = x7 + in[7];
    out[8] = x8 + in[8]; out[9] = x9 + in[9]; out[10] = x10 + in[10]; out[11] = x11 + in[11];
    out[12] = x12 + in[12]; out[13] = x13 + in[13]; out[14] = x14 + in[14]; out[15] = x15 + in[15];
}
#undef CIRCL_CHACHA_QR

// RFC 8439 2.5 on 26-bit limbs
struct Poly1305 {
    uint32_t r[5], h[5], pad[4];

    // key = r || s as 8 little-endian words; r is clamped here
    CIRCL_HD void init(const uint32_t *key) {
        r[0] = key[0] & 0x3ffffffu;
        r[1] = ((key[0] >> 26) | (key[1] << 6)) & 0x3ffff03u;
        r[2] = ((key[1] >> 20) | (key[2] << 12)) & 0x3ffc0ffu;
        r[3] = ((key[2] >> 14) | (key[3] << 18)) & 0x3f03fffu;
        r[4] = (key[3] >> 8) & 0x00fffffu;
        for (int i = 0; i < 5; i++) h[i] = 0;
        for (int i = 0; i < 4; i++) pad[i] = key[4 + i];
    }
    // h = (h + m + hibit * 2^128) * r mod 2^130 - 5, partially reduced; m = 16 bytes as 4 little-endian words
    CIRCL_HD void block(const uint32_t *m, uint32_t hibit = 1) {
        const uint32_t s1 = r[1] * 5, s2 = r[2] * 5, s3 = r[3] * 5, s4 = r[4] * 5;
        const uint64_t h0 = h[0] + (m[0] & 0x3ffffffu);
        const uint64_t h1 = h[1] + (((m[0] >> 26) | (m[1] << 6)) & 0x3ffffffu);
        const uint64_t h2 = h[2] + (((m[1] >> 20) | (m[2] << 12)) & 0x3ffffffu);
        const uint64_t h3 = h[3] + (((m[2] >> 14) | (m[3] << 18)) & 0x3ffffffu);
        const uint64_t h4 = h[4] + ((m[3] >> 8) | (hibit << 24));
        uint64_t d0 = h0 * r[0] + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
        uint64_t d1 = h0 * r[1] + h1 * r[0] + h2 * s4 + h3 * s3 + h4 * s2;
        uint64_t d2 = h0 * r[2] + h1 * r[1] + h2 * r[0] + h3 * s4 + h4 * s3;
        uint64_t d3 = h0 * r[3] + h1 * r[2] + h2 * r[1] + h3 * r[0] + h4 * s4;
        uint64_t d4 = h0 * r[4] + h1 * r[3] + h2 * r[2] + h3 * r[1] + h4 * r[0];
        uint64_t c;
        c = d0 >> 26; h[0] = (uint32_t)d0 & 0x3ffffffu; d1 += c;
        c = d1 >> 26; h[1] = (uint32_t)d1 & 0x3ffffffu; d2 += c;
        c = d2 >> 26; h[2] = (uint32_t)d2 & 0x3ffffffu; d3 += c;
        c = d3 >> 26; h[3] = (uint32_t)d3 & 0x3ffffffu; d4 += c;
        c = d4 >> 26; h[4] = (uint32_t)d4 & 0x3ffffffu;
        h[0] += (uint32_t)c * 5;
        h[1] += h[0] >> 26;
        h[0] &= 0x3ffffffu;
    }
    // tag = ((h mod 2^130 - 5) + s) mod 2^128 as 4 little-endian words
    CIRCL_HD void finish(uint32_t *tag) {
        uint32_t c;
        c = h[1] >> 26; h[1] &= 0x3ffffffu; h[2] += c;
        c = h[2] >> 26; h[2] &= 0x3ffffffu; h[3] += c;
        c = h[3] >> 26; h[3] &= 0x3ffffffu; h[4] += c;
        c = h[4] >> 26; h[4] &= 0x3ffffffu; h[0] += c * 5;
        c = h[0] >> 26; h[0] &= 0x3ffffffu; h[1] += c;
        // g = h + 5 - 2^130: h >= p exactly when this does not borrow
        uint32_t g[5];
        g[0] = h[0] + 5; c = g[0] >> 26; g[0] &= 0x3ffffffu;
        g[1] = h[1] + c; c = g[1] >> 26; g[1] &= 0x3ffffffu;
        g[2] = h[2] + c; c = g[2] >> 26; g[2] &= 0x3ffffffu;
        g[3] = h[3] + c; c = g[3] >> 26; g[3] &= 0x3ffffffu;
        g[4] = h[4] + c - (1u << 26);
        const uint32_t take_g = (g[4] >> 31) - 1u;  // all ones if h >= p
        for (int i = 0; i < 5; i++) h[i] = (h[i] & ~take_g) | (g[i] & take_g);
        h[4] &= 0x3ffffffu;
        const uint32_t w0 = h[0] | (h[1] << 26), w1 = (h[1] >> 6) | (h[2] << 20), w2 = (h[2] >> 12) | (h[3] << 14), w3 = (h[3] >> 18) | (h[4] << 8);
        uint64_t f;
        f = (uint64_t)w0 + pad[0]; tag[0] = (uint32_t)f;
        f = (uint64_t)w1 + pad[1] + (f >> 32); tag[1] = (uint32_t)f;
        f = (uint64_t)w2 + pad[2] + (f >> 32); tag[2] = (uint32_t)f;
        f = (uint64_t)w3 + pad[3] + (f >> 32); tag[3] = (uint32_t)f;
    }
};

// the up to 16 bytes p[0 .. nb) as 4 little-endian words, zeros behind them
CIRCL_HD void load_chunk(uint32_t *w, const uint8_t *p, uint32_t nb) {
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((uint32_t)k < nb) w[k / 4] |= (uint32_t)p[k] << (8 * (k % 4));
}
CIRCL_HD void store_chunk(uint8_t *p, const uint32_t *w, uint32_t nb) {
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((uint32_t)k < nb) p[k] = (uint8_t)(w[k / 4] >> (8 * (k % 4)));
}

// the range p[0 .. len), zero-padded to a multiple of 16, into the MAC (RFC 8439 2.8)
CIRCL_HD void mac_padded(Poly1305 &mac, const uint8_t *p, uint64_t len) {
    for (uint64_t o = 0; o < len; o += 16) {
        uint32_t w[4];
        load_chunk(w, p + o, len - o < 16 ? (uint32_t)(len - o) : 16u);
        mac.block(w);
    }
}
CIRCL_HD void mac_lengths(Poly1305 &mac, uint64_t aad_len, uint64_t ct_len) {
    const uint32_t w[4] = {(uint32_t)aad_len, (uint32_t)(aad_len >> 32), (uint32_t)ct_len, (uint32_t)(ct_len >> 32)};
    mac.block(w);
}

// dst[0 .. len) = (src ^ keystream from block `counter` on) & mask; with MAC_DST the written bytes also enter the MAC (Seal)
template <bool MAC_DST>
CIRCL_HD void xor_stream(uint8_t *dst, const uint8_t *src, uint64_t len, const uint32_t *key, const uint32_t *nonce, uint32_t mask, Poly1305 &mac) {
    uint32_t counter = 1;
    for (uint64_t o = 0; o < len; o += 64, counter++) {
        uint32_t ks[16];
        chacha20_block(ks, key, counter, nonce);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint64_t at = o + 16 * q;
            if (at < len) {
                const uint32_t nb = len - at < 16 ? (uint32_t)(len - at) : 16u;
                uint32_t w[4];
                load_chunk(w, src + at, nb);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t keep = nb >= 4u * j + 4 ? 0xffffffffu : nb > 4u * j ? (1u << (8 * (nb - 4u * j))) - 1u : 0u;
                    w[j] = (w[j] ^ ks[4 * q + j]) & keep & mask;
                }
                store_chunk(dst + at, w, nb);
                if (MAC_DST) mac.block(w);
            }
        }
    }
}

// the nonce of sequence number seq (aead.go:47-52): base_nonce XOR BE96(seq), as 3 little-endian words
CIRCL_HD void seq_nonce(uint32_t *nonce, const uint32_t *base_nonce, uint64_t seq) {
    nonce[0] = base_nonce[0];
    nonce[1] = base_nonce[1] ^ hkdf::bswap32((uint32_t)(seq >> 32));
    nonce[2] = base_nonce[2] ^ hkdf::bswap32((uint32_t)seq);
}

// ct[0 .. pt_len + 16) = Seal(key, nonce, pt, aad), every byte ANDed with mask (all ones, or 0 for an item that failed before)
CIRCL_HD void seal(uint8_t *ct, const uint32_t *key, const uint32_t *nonce, const uint8_t *pt, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len,
                   uint32_t mask) {
    uint32_t b0[16], tag[4];
    chacha20_block(b0, key, 0, nonce);
    Poly1305 mac;
    mac.init(b0);
    mac_padded(mac, aad, aad_len);
    xor_stream<true>(ct, pt, pt_len, key, nonce, 0xffffffffu, mac);
    mac_lengths(mac, aad_len, pt_len);
    mac.finish(tag);
    if (mask != 0xffffffffu) {  // (public: ok is an output) the row was written unmasked so that the MAC saw the ciphertext
        for (uint64_t o = 0; o < pt_len; o++) ct[o] = 0;
    }
    for (int j = 0; j < 4; j++) tag[j] &= mask;
    store_chunk(ct + pt_len, tag, 16);
}

// pt[0 .. pt_len) = Open(key, nonce, ct[0 .. pt_len + 16), aad); returns 1, or 0 with an all-zero pt.  `good` = the item's verdict
// so far (0 or 1): a 0 gives 0.
CIRCL_HD uint32_t open(uint8_t *pt, const uint32_t *key, const uint32_t *nonce, const uint8_t *ct, uint64_t pt_len, const uint8_t *aad, uint64_t aad_len,
                       uint32_t good) {
    uint32_t b0[16], tag[4], got[4];
    chacha20_block(b0, key, 0, nonce);
    Poly1305 mac;
    mac.init(b0);
    mac_padded(mac, aad, aad_len);
    mac_padded(mac, ct, pt_len);
    mac_lengths(mac, aad_len, pt_len);
    mac.finish(tag);
    load_chunk(got, ct + pt_len, 16);
    const uint32_t diff = (tag[0] ^ got[0]) | (tag[1] ^ got[1]) | (tag[2] ^ got[2]) | (tag[3] ^ got[3]);
    good &= 1u ^ ((diff | (0u - diff)) >> 31);
    xor_stream<false>(pt, ct, pt_len, key, nonce, 0u - good, mac);
    return good;
}

}  // namespace chapoly
}  // namespace circl
