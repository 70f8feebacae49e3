// tests/hostsim/hpke_ctx_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/hkdf_stream_dev.h, chacha20poly1305_dev.h and hpke_kernels.h on the CPU (their host instantiation), so that the
// CPU-only test tier can check the very source the HPKE context kernels are built from against hmac and tests/hpke_ctx.py.
// Nothing here is linked into libcirclhip.so.
//
// With -DHPKE_CTX_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: it runs ragged batches whose blobs are heap
// blocks of exactly their size through setup, Seal, Open and Export on both sides and checks that the two sides agree.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hpke_kernels.h"

using namespace circl;
using dhkem::X25519;
using dhkem::X448;
using hkdf::Sha256;
using hkdf::Sha512;

extern "C" {

// kdf: 1 = HKDF-SHA256, 3 = HKDF-SHA512
void hs_hmac_stream(int kdf, uint32_t *out, const uint32_t *key, int key_words, const uint8_t *a, uint32_t alen, const uint8_t *b, uint64_t blen,
                    const uint8_t *c, uint32_t clen) {
    if (kdf == 1) hkdf::hmac_stream<Sha256>(out, key, key_words, a, alen, b, blen, c, clen);
    else hkdf::hmac_stream<Sha512>(out, key, key_words, a, alen, b, blen, c, clen);
}

// LabeledExpand(prk, "sec", info, L) for the suite (kem, kdf, aead)
void hs_labeled_expand_stream(int kem, int kdf, int aead, uint8_t *out, uint32_t L, const uint32_t *prk, const uint8_t *info, uint64_t info_len) {
    const hkdf::SuiteId id = {kem, kdf, aead};
    if (kdf == 1) hkdf::labeled_expand_stream<Sha256>(out, L, prk, id, "sec", info, info_len, 0xff);
    else hkdf::labeled_expand_stream<Sha512>(out, L, prk, id, "sec", info, info_len, 0xff);
}

// RFC 8439 2.5 on a whole message: a partial last block gets its 01 byte and no 2^128
void hs_poly1305(uint32_t *tag, const uint32_t *key, const uint8_t *msg, uint64_t len) {
    chapoly::Poly1305 mac;
    mac.init(key);
    for (uint64_t o = 0; o < len; o += 16) {
        uint32_t w[4];
        const uint32_t nb = len - o < 16 ? (uint32_t)(len - o) : 16u;
        chapoly::load_chunk(w, msg + o, nb);
        if (nb < 16) w[nb / 4] |= 1u << (8 * (nb % 4));
        mac.block(w, nb == 16);
    }
    mac.finish(tag);
}

void hs_chacha20_block(uint32_t *out, const uint32_t *key, uint32_t counter, const uint32_t *nonce) { chapoly::chacha20_block(out, key, counter, nonce); }

int hs_setup_item(int sender, const hpke::SetupArgs *a, uint64_t i) {
    const bool x255 = a->kem == 0x20, s256 = a->kdf == 1;
    if (sender) {
        if (x255 && s256) hpke::setup_item<X25519, Sha256, true>(*a, i);
        else if (x255) hpke::setup_item<X25519, Sha512, true>(*a, i);
        else if (s256) hpke::setup_item<X448, Sha256, true>(*a, i);
        else hpke::setup_item<X448, Sha512, true>(*a, i);
    } else {
        if (x255 && s256) hpke::setup_item<X25519, Sha256, false>(*a, i);
        else if (x255) hpke::setup_item<X25519, Sha512, false>(*a, i);
        else if (s256) hpke::setup_item<X448, Sha256, false>(*a, i);
        else hpke::setup_item<X448, Sha512, false>(*a, i);
    }
    return 0;
}

void hs_aead_item(int seal, const hpke::AeadArgs *a, uint64_t i) {
    if (seal) hpke::aead_item<true>(*a, i);
    else hpke::aead_item<false>(*a, i);
}

void hs_export_item(const hpke::ExportArgs *a, uint64_t i) {
    if (a->kdf == 1) hpke::export_item<Sha256>(*a, i);
    else hpke::export_item<Sha512>(*a, i);
}

}  // extern "C"

#ifdef HPKE_CTX_HOSTSIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// a ragged array whose blob is a heap block of exactly its size (so that a sanitizer sees any read past a row's end)
struct Rag {
    uint8_t *blob = nullptr;
    std::vector<uint64_t> off;
    Rag(size_t n, size_t (*len)(size_t), uint32_t seed) : off(n + 1, 0) {
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + len(i);
        blob = static_cast<uint8_t *>(malloc(off[n] ? off[n] : 1));
        for (uint64_t k = 0; k < off[n]; k++) blob[k] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    }
    ~Rag() { free(blob); }
    Rag(const Rag &) = delete;
};

int fail(const char *what, int kem, int kdf, int mode) {
    printf("FAIL %s (kem 0x%x kdf %d mode %d)\n", what, kem, kdf, mode);
    return 1;
}

int run(int kem, int kdf, int aead, int mode) {
    const size_t n = 70, W = kem == 0x20 ? 8 : 14, CW = 12 + (kdf == 1 ? 8 : 16);
    const uint32_t L = 77;
    Rag info(n, [](size_t i) { return i + 20; }, 1), psk(n, [](size_t i) { return 32 + i % 40; }, 2), psk_id(n, [](size_t i) { return 1 + i % 30; }, 3);
    Rag pt(n, [](size_t i) { return i; }, 4), aad(n, [](size_t i) { return i % 41; }, 5), exp(n, [](size_t i) { return (i * 7) % 150; }, 6);
    Rag rows(5, [](size_t) { return size_t(70 * 56); }, 7);
    const bool has_psk = mode & 1, auth = mode & 2;
    std::vector<uint32_t> ikmE(n * W), skR(n * W), pkR(n * W), skS(n * W), pkS(n * W), enc(n * W), ctxS(n * CW), ctxR(n * CW);
    memcpy(ikmE.data(), rows.blob + rows.off[0], n * W * 4);
    memcpy(skR.data(), rows.blob + rows.off[1], n * W * 4);
    memcpy(skS.data(), rows.blob + rows.off[2], n * W * 4);
    for (size_t i = 0; i < n; i++) {
        if (kem == 0x20) { dhkem::X25519::base(&pkR[i * W], &skR[i * W]); dhkem::X25519::base(&pkS[i * W], &skS[i * W]); }
        else { dhkem::X448::base(&pkR[i * W], &skR[i * W]); dhkem::X448::base(&pkS[i * W], &skS[i * W]); }
    }
    std::vector<uint8_t> okS(n), okR(n), okO(n);
    hpke::SetupArgs s = {};
    s.pkR = pkR.data(); s.ikmE = ikmE.data(); s.skS = auth ? skS.data() : nullptr; s.enc_out = enc.data();
    s.info = info.blob; s.info_off = info.off.data();
    if (has_psk) { s.psk = psk.blob; s.psk_off = psk.off.data(); s.psk_id = psk_id.blob; s.psk_id_off = psk_id.off.data(); }
    s.ok = okS.data(); s.kem = kem; s.kdf = kdf; s.aead = aead; s.mode = mode; s.what = hpke::kStoreContext;
    s.ctx = ctxS.data(); s.ctx_stride_words = CW; s.n = n;
    hpke::SetupArgs r = s;
    r.pkR = nullptr; r.ikmE = nullptr; r.skS = nullptr; r.enc_out = nullptr;
    r.skR = skR.data(); r.enc_in = enc.data(); r.pkS = auth ? pkS.data() : nullptr; r.ok = okR.data(); r.ctx = ctxR.data();
    for (size_t i = 0; i < n; i++) { hs_setup_item(1, &s, i); hs_setup_item(0, &r, i); }
    if (memcmp(ctxS.data(), ctxR.data(), n * CW * 4)) return fail("the two sides' contexts differ", kem, kdf, mode);
    for (size_t i = 0; i < n; i++)
        if (!okS[i] || !okR[i]) return fail("setup refused an item", kem, kdf, mode);
    // Export on both sides
    uint8_t *outS = static_cast<uint8_t *>(malloc(n * L)), *outR = static_cast<uint8_t *>(malloc(n * L));
    hpke::ExportArgs e = {ctxS.data(), CW, kem, kdf, aead, exp.blob, exp.off.data(), L, outS, n};
    hpke::ExportArgs e2 = e;
    e2.ctx = ctxR.data(); e2.out = outR;
    for (size_t i = 0; i < n; i++) { hs_export_item(&e, i); hs_export_item(&e2, i); }
    const bool exp_same = !memcmp(outS, outR, n * L);
    free(outS); free(outR);
    if (!exp_same) return fail("the two sides' exports differ", kem, kdf, mode);
    if (aead == hpke::AEAD_EXPORT_ONLY) return 0;
    // Seal on stored rows, Open on the receiver's; then the single-shot forms
    const size_t ct_bytes = pt.off[n] + 16 * n;
    uint8_t *ct = static_cast<uint8_t *>(malloc(ct_bytes)), *ct1 = static_cast<uint8_t *>(malloc(ct_bytes)), *back = static_cast<uint8_t *>(malloc(pt.off[n] ? pt.off[n] : 1));
    std::vector<uint64_t> seq(n);
    for (size_t i = 0; i < n; i++) seq[i] = i * 0x0101010101ull;
    hpke::AeadArgs se = {ctxS.data(), CW, seq.data(), pt.blob, aad.blob, pt.off.data(), aad.off.data(), ct, nullptr, n};
    hpke::AeadArgs op = {ctxR.data(), CW, seq.data(), ct, aad.blob, pt.off.data(), aad.off.data(), back, okO.data(), n};
    int bad = 0;
    for (size_t i = 0; i < n; i++) { hs_aead_item(1, &se, i); hs_aead_item(0, &op, i); bad |= !okO[i]; }
    if (bad || memcmp(back, pt.blob, pt.off[n])) bad = fail("Open does not return Seal's plaintext", kem, kdf, mode);
    if (!bad) {
        ct[ct_bytes - 1] ^= 1;  // the last item's tag
        hs_aead_item(0, &op, n - 1);
        for (uint64_t k = pt.off[n - 1]; k < pt.off[n]; k++) bad |= back[k];
        if (okO[n - 1] || bad) bad = fail("a forged tag opens", kem, kdf, mode);
    }
    if (!bad) {
        s.what = hpke::kAead; s.in = pt.blob; s.aad = aad.blob; s.pt_off = pt.off.data(); s.aad_off = aad.off.data(); s.out = ct1; s.ctx = nullptr;
        r.what = hpke::kAead; r.in = ct1; r.aad = aad.blob; r.pt_off = pt.off.data(); r.aad_off = aad.off.data(); r.out = back; r.ctx = nullptr;
        memset(back, 0xa5, pt.off[n]);
        for (size_t i = 0; i < n; i++) { hs_setup_item(1, &s, i); hs_setup_item(0, &r, i); bad |= !okR[i]; }
        if (bad || memcmp(back, pt.blob, pt.off[n])) bad = fail("single-shot Open does not return single-shot Seal's plaintext", kem, kdf, mode);
    }
    free(ct); free(ct1); free(back);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    for (int kem : {0x20, 0x21})
        for (int kdf : {1, 3}) {
            bad |= run(kem, kdf, 3, 0);
            bad |= run(kem, kdf, 3, 3);
            bad |= run(kem, kdf, 0xffff, 1);
        }
    // the byte-ragged primitives at every length, on exact-size blocks
    for (int kdf : {1, 3})
        for (size_t len = 0; len <= 300; len++) {
            uint8_t *m = static_cast<uint8_t *>(malloc(len ? len : 1));
            memset(m, (int)len, len);
            uint32_t out[16], key[16] = {1, 2, 3};
            hs_hmac_stream(kdf, out, key, 8, m, (uint32_t)(len / 3), m + len / 3, len - len / 3, nullptr, 0);
            free(m);
        }
    puts(bad ? "hpke_ctx_hostsim: FAILED" : "hpke_ctx_hostsim: ok");
    return bad;
}
#endif
