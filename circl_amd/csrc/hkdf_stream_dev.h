// hkdf_stream_dev.h -- HMAC and HKDF (RFC 5869) over messages whose length is known only at run time, on the two hash policies of
// hkdf_dev.h, and on top of them HPKE's LabeledExtract / LabeledExpand for a suite (hpke/util.go:73-107), one computation per lane.
//
// hkdf_dev.h builds every message in registers because the KEM's messages have fixed shapes.  The key schedule hashes what the
// caller brings -- info, psk, psk_id, an exporter context -- so a message here is three byte ranges one after the other: a short
// head the lane built itself (a T(i - 1) block, BE16(L), the labelled header), a body (caller's bytes in global memory, or the
// lane's own key_schedule_context) and a tail (the counter byte of Expand).  The lengths are public, so they steer loops; the
// bytes are absorbed one at a time into a block buffer that is compressed when it is full.  Keys and pseudorandom keys are word
// arrays of the lane.  An HMAC is a function of its own (CIRCL_HKDF_STREAM_CALL), so that a key schedule of six of them carries one
// copy of the compression per hash.
#pragma once
#include <stdint.h>

#include "hkdf_dev.h"

// WV: the waves per SIMD (amdgpu_waves_per_eu) of the kernels that call it.  A function of its own is allocated registers on its
// own, within the loosest bound among the kernels that reach it, and a kernel's occupancy is that of the greediest function it
// reaches.  WV only tells the copies apart: the X25519 kernels (4 waves) and the X448 kernels (2) each reach their own, so a
// compression is held to 128 registers beside the X25519 ladder instead of halving the occupancy that ladder runs at.
#define CIRCL_HKDF_STREAM_CALL(WV) static __host__ __device__ __attribute__((noinline))

namespace circl {
namespace hkdf {

// one compression as a call: the streams below meet a block boundary in several places and share this copy
template <class H, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void block_call(typename H::State &s, const uint32_t *m) {
    H::block(s, m);
}

// a hash in progress: BLOCK bytes of buffer as little-endian words (the layout H::block takes), compressed whenever they fill up
template <class H, int WV>
struct Stream {
    static constexpr int BW = H::BLOCK / 4;
    typename H::State s;
    uint32_t buf[BW];
    uint32_t pos;    // bytes in buf
    uint64_t total;  // bytes absorbed

    CIRCL_HD void init() {
        H::init(s);
        for (int i = 0; i < BW; i++) buf[i] = 0;
        pos = 0;
        total = 0;
    }
    CIRCL_HD void flush() {
        block_call<H, WV>(s, buf);
        for (int i = 0; i < BW; i++) buf[i] = 0;
        pos = 0;
    }
    CIRCL_HD void put(uint8_t b) {
        buf[pos >> 2] |= (uint32_t)b << (8 * (pos & 3));
        total++;
        if (++pos == (uint32_t)H::BLOCK) flush();
    }
    CIRCL_HD void put(const uint8_t *p, uint64_t len) {
        for (uint64_t i = 0; i < len; i++) put(p[i]);
    }
    // a whole block of words at a block boundary (the key block of an HMAC)
    CIRCL_HD void put_block(const uint32_t *w) {
        block_call<H, WV>(s, w);
        total += H::BLOCK;
    }
    CIRCL_HD void finish(uint32_t *out) {
        buf[pos >> 2] |= 0x80u << (8 * (pos & 3));
        if (pos + 1 + H::LEN_BYTES > (uint32_t)H::BLOCK) flush();
        buf[BW - 2] = bswap32((uint32_t)(total >> 29));
        buf[BW - 1] = bswap32((uint32_t)(total << 3));
        block_call<H, WV>(s, buf);
        H::digest(out, s);
    }
};

// out = HMAC(key, a || b || c): key = key_words <= BLOCK / 4 words (0: the zero key of an Extract with the empty salt); any of
// the three ranges may be empty (then its pointer is not read).  out = H::OUT / 4 words.
template <class H, int WV = 4>
CIRCL_HKDF_STREAM_CALL(WV) void hmac_stream(uint32_t *out, const uint32_t *key, int key_words, const uint8_t *a, uint32_t alen, const uint8_t *b, uint64_t blen,
                                        const uint8_t *c, uint32_t clen) {
    constexpr int BW = H::BLOCK / 4, OW = H::OUT / 4;
    uint32_t kb[BW];
    for (int i = 0; i < BW; i++) kb[i] = (i < key_words ? key[i] : 0u) ^ 0x36363636u;
    Stream<H, WV> st;
    st.init();
    st.put_block(kb);
    st.put(a, alen);
    st.put(b, blen);
    st.put(c, clen);
    uint32_t inner[OW];
    st.finish(inner);
    for (int i = 0; i < BW; i++) kb[i] ^= 0x36363636u ^ 0x5c5c5c5cu;
    st.init();
    st.put_block(kb);
    st.put(reinterpret_cast<const uint8_t *>(inner), H::OUT);
    st.finish(out);
    for (int i = 0; i < BW; i++) kb[i] = 0;
}

// uniform = expand_message_xmd(H, pre || body || suf, dst, out_len) (RFC 9380 5.3.1), as words the way memory holds them; out has room
// for ell = ceil(out_len / H::OUT) <= 3 digests:
//   b_0 = H(0^BLOCK || msg || I2OSP(out_len, 2) || 0 || DST'),  b_1 = H(b_0 || 1 || DST'),  b_i = H((b_0 xor b_(i-1)) || i || DST')
// pre and suf are bytes the lane built, body is the caller's bytes in global memory.  1 <= len(DST) <= 255 (RFC 9380's rule for a longer
// DST is not implemented: the entry points refuse it).  A function of its own per hash and occupancy class, as the streams are.
template <class H, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void xmd(uint32_t *out, uint32_t out_len, const uint8_t *pre, uint32_t pre_len, const uint8_t *body, uint64_t body_len,
                                    const uint8_t *suf, uint32_t suf_len, const uint8_t *dst, uint32_t dst_len) {
    constexpr int OW = H::OUT / 4;
    Stream<H, WV> st;
    uint32_t zero[H::BLOCK / 4], b0[OW], x[OW];
    for (int i = 0; i < H::BLOCK / 4; i++) zero[i] = 0;
    st.init();
    st.put_block(zero);
    st.put(pre, pre_len);
    st.put(body, body_len);
    st.put(suf, suf_len);
    st.put((uint8_t)(out_len >> 8));
    st.put((uint8_t)out_len);
    st.put((uint8_t)0);
    st.put(dst, dst_len);
    st.put((uint8_t)dst_len);
    st.finish(b0);
    const uint32_t ell = (out_len + H::OUT - 1) / H::OUT;
    for (uint32_t i = 1; i <= ell; i++) {
        for (int j = 0; j < OW; j++) x[j] = i == 1 ? b0[j] : b0[j] ^ out[(i - 2) * OW + j];
        st.init();
        st.put(reinterpret_cast<const uint8_t *>(x), H::OUT);
        st.put((uint8_t)i);
        st.put(dst, dst_len);
        st.put((uint8_t)dst_len);
        st.finish(out + (i - 1) * OW);
    }
    for (int j = 0; j < OW; j++) b0[j] = x[j] = 0;
}

// the HPKE suite of a context (util.go:85-91): the three code points that enter every label
struct SuiteId {
    int kem, kdf, aead;
};

constexpr int LABEL_HEAD_MAX = 2 + 7 + 10 + 16;  // BE16(L) || "HPKE-v1" || suite_id || room for the longest label

// "HPKE-v1" || "HPKE" || BE16(kem) || BE16(kdf) || BE16(aead) || label at m; returns the bytes written (17 + the label's length)
template <int LN>
CIRCL_HD int put_labeled_head(uint8_t *m, SuiteId id, const char (&label)[LN]) {
    static_assert(LN - 1 <= 16, "labels are short");
    const char v[] = "HPKE-v1HPKE";
    for (int i = 0; i < 11; i++) m[i] = (uint8_t)v[i];
    m[11] = (uint8_t)(id.kem >> 8); m[12] = (uint8_t)id.kem;
    m[13] = (uint8_t)(id.kdf >> 8); m[14] = (uint8_t)id.kdf;
    m[15] = (uint8_t)(id.aead >> 8); m[16] = (uint8_t)id.aead;
    for (int i = 0; i < LN - 1; i++) m[17 + i] = (uint8_t)label[i];
    return 17 + LN - 1;
}

// util.go:73-83 labeledExtract: prk = HMAC(salt, "HPKE-v1" || suite_id || label || ikm); salt = salt_words words (0: empty)
template <class H, int WV = 4, int LN>
CIRCL_HD void labeled_extract_stream(uint32_t *prk, SuiteId id, const uint32_t *salt, int salt_words, const char (&label)[LN], const uint8_t *ikm,
                                     uint64_t ikm_len) {
    uint8_t head[LABEL_HEAD_MAX];
    const int n = put_labeled_head(head, id, label);
    hmac_stream<H, WV>(prk, salt, salt_words, head, (uint32_t)n, ikm, ikm_len, nullptr, 0);
}

// util.go:93-107 labeledExpand for any 0 < L <= 255 * H::OUT: out[0 .. L) = T(1) || T(2) || ..., T(i) = HMAC(prk, T(i - 1) ||
// BE16(L) || "HPKE-v1" || suite_id || label || info || i).  Every byte is ANDed with mask8 (0xff, or 0 for a failed item).
template <class H, int WV = 4, int LN>
CIRCL_HD void labeled_expand_stream(uint8_t *out, uint32_t L, const uint32_t *prk, SuiteId id, const char (&label)[LN], const uint8_t *info, uint64_t info_len,
                                    uint8_t mask8) {
    constexpr int OW = H::OUT / 4;
    uint32_t head[(H::OUT + LABEL_HEAD_MAX + 3) / 4], t[OW];
    uint8_t *hb = reinterpret_cast<uint8_t *>(head);
    uint8_t *lab = hb + H::OUT;  // T(i - 1) sits in front of it from the second block on
    lab[0] = (uint8_t)(L >> 8);
    lab[1] = (uint8_t)L;
    const int n = 2 + put_labeled_head(lab + 2, id, label);
    uint32_t done = 0;
    for (uint32_t i = 1; done < L; i++) {
        const uint8_t ctr = (uint8_t)i;
        if (i == 1) hmac_stream<H, WV>(t, prk, OW, lab, (uint32_t)n, info, info_len, &ctr, 1);
        else hmac_stream<H, WV>(t, prk, OW, hb, (uint32_t)(H::OUT + n), info, info_len, &ctr, 1);
        for (int j = 0; j < OW; j++) head[j] = t[j];
        const uint32_t take = L - done < (uint32_t)H::OUT ? L - done : (uint32_t)H::OUT;
        for (uint32_t j = 0; j < take; j++) out[done + j] = (uint8_t)(t[j >> 2] >> (8 * (j & 3))) & mask8;
        done += take;
    }
}

}  // namespace hkdf
}  // namespace circl
