// hpke_kernels.h -- batch HPKE contexts (RFC 9180 sections 5 and 6; hpke/hpke.go, hpke/util.go, hpke/aead.go) over the DHKEMs of
// dhkem_kernels.h, HKDF-SHA256 / HKDF-SHA512 and ChaCha20-Poly1305 (or export-only): one item per lane, no workspace.
//
// A setup is the KEM operation (op_encap / op_auth_encap for a sender, op_decap / op_auth_decap for a receiver), the key schedule
// on its shared secret, and then ONE of three endings, chosen per launch: the context row is stored (Setup), or it is used at once
// for a Seal / Open at sequence number 0 or for an Export (the single-shot forms of RFC 9180 section 6) and never stored.  Either
// way the shared secret stays in the lane.  Seal, Open and Export on stored context rows are kernels of their own.
//
// A context row is key[32] || base_nonce[12] || 0[4] || exporter_secret[Nh] (48 + Nh bytes, 4-byte aligned); key and base_nonce
// are zero for the export-only AEAD.
//
// The KEM operation and the key schedule are functions of their own (CIRCL_HPKE_CALL): the scalar multiplications inside the KEM
// operation keep the register allocation they have in dhkem_kernels.h, and what the key schedule and the AEAD hold does not live
// across them.  Each is instantiated per occupancy class (C::WAVES), so that hashing is allocated within the
// registers of the kernel's own occupancy and does not lower the occupancy the ladder runs at.  Failure (a low-order point, a psk that verifyPSKInputs refuses, a tag that does not verify) is a mask: ok = 0 and
// every output row of the item is zero.
#pragma once
#include <hip/hip_runtime.h>

#include "chacha20poly1305_dev.h"
#include "dhkem_kernels.h"
#include "hkdf_stream_dev.h"

#define CIRCL_HPKE_CALL(WV) static __host__ __device__ __attribute__((noinline))  // WV: as in hkdf_stream_dev.h

namespace circl {
namespace hpke {

using hkdf::SuiteId;

constexpr int AEAD_CHACHA20POLY1305 = 0x0003, AEAD_EXPORT_ONLY = 0xffff;
constexpr int CTX_HEAD_WORDS = 12;  // key || base_nonce || 0
constexpr int EXPORT_WAVES = 4;    // the Export kernel on context rows: hashing only

// item i of a ragged array: blob == nullptr or off == nullptr means every item is empty
CIRCL_HD uint64_t off_at(const uint64_t *off, size_t i) { return off ? off[i] : 0; }
CIRCL_HD uint64_t range_of(const uint8_t *&p, const uint8_t *blob, const uint64_t *off, size_t i) {
    if (!blob || !off) {
        p = nullptr;
        return 0;
    }
    p = blob + off[i];
    return off[i + 1] - off[i];
}

// util.go:9-71 keySchedule: ctx = CTX_HEAD_WORDS + HK::OUT / 4 words (the context row); ss = the KEM's shared secret.  Returns
// verifyPSKInputs' verdict (1 / 0); the row is computed either way and the caller masks it.
template <class HK, int WV>
CIRCL_HPKE_CALL(WV) uint32_t key_schedule(uint32_t *ctx, const uint32_t *ss, int ss_words, SuiteId id, int mode, const uint8_t *info, uint64_t info_len,
                                      const uint8_t *psk, uint64_t psk_len, const uint8_t *psk_id, uint64_t psk_id_len) {
    constexpr int OW = HK::OUT / 4, KSC = 1 + 2 * HK::OUT;
    const bool want_psk = (mode & 1) != 0;
    const uint32_t good = (psk_len != 0) == want_psk && (psk_id_len != 0) == want_psk;
    uint32_t t[OW], secret[OW], kscw[(KSC + 3) / 4];
    uint8_t *ksc = reinterpret_cast<uint8_t *>(kscw);
    ksc[0] = (uint8_t)mode;
    hkdf::labeled_extract_stream<HK, WV>(t, id, nullptr, 0, "psk_id_hash", psk_id, psk_id_len);
    for (int j = 0; j < HK::OUT; j++) ksc[1 + j] = (uint8_t)(t[j >> 2] >> (8 * (j & 3)));
    hkdf::labeled_extract_stream<HK, WV>(t, id, nullptr, 0, "info_hash", info, info_len);
    for (int j = 0; j < HK::OUT; j++) ksc[1 + HK::OUT + j] = (uint8_t)(t[j >> 2] >> (8 * (j & 3)));
    hkdf::labeled_extract_stream<HK, WV>(secret, id, ss, ss_words, "secret", psk, psk_len);
    for (int j = 0; j < CTX_HEAD_WORDS; j++) ctx[j] = 0;
    uint8_t *row = reinterpret_cast<uint8_t *>(ctx);
    if (id.aead != AEAD_EXPORT_ONLY) {
        hkdf::labeled_expand_stream<HK, WV>(row, 32, secret, id, "key", ksc, KSC, 0xff);
        hkdf::labeled_expand_stream<HK, WV>(row + 32, 12, secret, id, "base_nonce", ksc, KSC, 0xff);
    }
    hkdf::labeled_expand_stream<HK, WV>(row + 4 * CTX_HEAD_WORDS, HK::OUT, secret, id, "exp", ksc, KSC, 0xff);
    for (int j = 0; j < OW; j++) secret[j] = t[j] = 0;
    return good;
}

// the KEM operation of a sender / a receiver; mode & 2: the authenticated one
template <class C>
CIRCL_HPKE_CALL(C::WAVES) uint32_t kem_send(int mode, const uint32_t *pkR, const uint32_t *ikmE, const uint32_t *skS, const uint32_t *pkS, uint32_t *enc, uint32_t *ss) {
    return (mode & 2) ? dhkem::op_auth_encap<C>(pkR, skS, pkS, ikmE, enc, ss) : dhkem::op_encap<C>(pkR, ikmE, enc, ss);
}
template <class C>
CIRCL_HPKE_CALL(C::WAVES) uint32_t kem_recv(int mode, const uint32_t *skR, const uint32_t *pkR, const uint32_t *enc, const uint32_t *pkS, uint32_t *ss) {
    return (mode & 2) ? dhkem::op_auth_decap<C>(skR, pkR, enc, pkS, ss) : dhkem::op_decap<C>(skR, pkR, enc, ss);
}

// what a setup launch does with the context
enum What : int { kStoreContext = 0, kAead = 1, kExport = 2 };

struct SetupArgs {
    // key rows of C::W words: a sender has pkR, ikmE, skS / pkS (auth modes; pkS may be nullptr) and writes enc; a receiver has skR,
    // pkR (may be nullptr), enc, pkS (auth modes)
    const uint32_t *pkR, *ikmE, *skR, *skS, *pkS;
    uint32_t *enc_out;
    const uint32_t *enc_in;
    const uint8_t *info, *psk, *psk_id;
    const uint64_t *info_off, *psk_off, *psk_id_off;
    uint8_t *ok;  // may be nullptr
    int kem, kdf, aead, mode, what;
    // kStoreContext
    uint32_t *ctx;
    size_t ctx_stride_words;
    // kAead: Seal (sender: in = pt, out = ct) or Open (receiver: in = ct, out = pt) at sequence number 0; item i's plaintext is
    // pt_off[i + 1] - pt_off[i] bytes at pt_off[i], its ciphertext 16 bytes longer at pt_off[i] + 16 i
    const uint8_t *in, *aad;
    const uint64_t *pt_off, *aad_off;
    uint8_t *out;
    // kExport: L bytes per item
    const uint8_t *exp;
    const uint64_t *exp_off;
    uint32_t L;
    uint8_t *exp_out;
    size_t n;
};

// one item of a setup launch
template <class C, class HK, bool SENDER>
CIRCL_HD void setup_item(const SetupArgs &a, size_t i) {
    constexpr int OW = HK::OUT / 4, SW = C::H::OUT / 4;
    const SuiteId id = {a.kem, a.kdf, a.aead};
    uint32_t ss[SW], ctx[CTX_HEAD_WORDS + OW];
    uint32_t good;
    if (SENDER)
        good = kem_send<C>(a.mode, a.pkR + i * C::W, a.ikmE + i * C::W, a.skS ? a.skS + i * C::W : nullptr, a.pkS ? a.pkS + i * C::W : nullptr,
                           a.enc_out + i * C::W, ss);
    else
        good = kem_recv<C>(a.mode, a.skR + i * C::W, a.pkR ? a.pkR + i * C::W : nullptr, a.enc_in + i * C::W, a.pkS ? a.pkS + i * C::W : nullptr, ss);
    const uint8_t *info, *psk, *psk_id;
    const uint64_t info_len = range_of(info, a.info, a.info_off, i), psk_len = range_of(psk, a.psk, a.psk_off, i),
                   psk_id_len = range_of(psk_id, a.psk_id, a.psk_id_off, i);
    const uint32_t psk_good = key_schedule<HK, C::WAVES>(ctx, ss, SW, id, a.mode, info, info_len, psk, psk_len, psk_id, psk_id_len);
    for (int j = 0; j < SW; j++) ss[j] = 0;
    if (SENDER && !psk_good) {  // (the lengths are public) the KEM has written enc under its own verdict only
        for (int j = 0; j < C::W; j++) a.enc_out[i * C::W + j] = 0;
    }
    good &= psk_good;
    const uint32_t mask = 0u - good;
    for (int j = 0; j < CTX_HEAD_WORDS + OW; j++) ctx[j] &= mask;
    if (a.what == kStoreContext) {
        for (int j = 0; j < CTX_HEAD_WORDS + OW; j++) a.ctx[i * a.ctx_stride_words + j] = ctx[j];
    } else if (a.what == kAead) {
        const uint8_t *aad;
        const uint64_t aad_len = range_of(aad, a.aad, a.aad_off, i);
        const uint64_t at = off_at(a.pt_off, i), pt_len = off_at(a.pt_off, i + 1) - at;
        if (SENDER) chapoly::seal(a.out + at + 16 * i, ctx, ctx + 8, a.in + at, pt_len, aad, aad_len, mask);
        else good = chapoly::open(a.out + at, ctx, ctx + 8, a.in + at + 16 * i, pt_len, aad, aad_len, good);
    } else {
        const uint8_t *exp;
        const uint64_t exp_len = range_of(exp, a.exp, a.exp_off, i);
        hkdf::labeled_expand_stream<HK, C::WAVES>(a.exp_out + i * (size_t)a.L, a.L, ctx + CTX_HEAD_WORDS, id, "sec", exp, exp_len, (uint8_t)mask);
    }
    if (a.ok) a.ok[i] = (uint8_t)good;
}

// ---- Seal / Open / Export on stored context rows ----------------------------------------------------------------------------
struct AeadArgs {
    const uint32_t *ctx;
    size_t ctx_stride_words;
    const uint64_t *seq;  // nullptr: 0
    const uint8_t *in, *aad;
    const uint64_t *pt_off, *aad_off;
    uint8_t *out, *ok;
    size_t n;
};

template <bool SEAL>
CIRCL_HD void aead_item(const AeadArgs &a, size_t i) {
    uint32_t key[8], nonce[3];
    const uint32_t *row = a.ctx + i * a.ctx_stride_words;
    for (int j = 0; j < 8; j++) key[j] = row[j];
    chapoly::seq_nonce(nonce, row + 8, a.seq ? a.seq[i] : 0);
    const uint8_t *aad;
    const uint64_t aad_len = range_of(aad, a.aad, a.aad_off, i);
    const uint64_t at = off_at(a.pt_off, i), pt_len = off_at(a.pt_off, i + 1) - at;
    if (SEAL) {
        chapoly::seal(a.out + at + 16 * i, key, nonce, a.in + at, pt_len, aad, aad_len, 0xffffffffu);
    } else {
        const uint32_t good = chapoly::open(a.out + at, key, nonce, a.in + at + 16 * i, pt_len, aad, aad_len, 1);
        if (a.ok) a.ok[i] = (uint8_t)good;
    }
}

struct ExportArgs {
    const uint32_t *ctx;
    size_t ctx_stride_words;
    int kem, kdf, aead;
    const uint8_t *exp;
    const uint64_t *exp_off;
    uint32_t L;
    uint8_t *out;
    size_t n;
};

// hpke.go Export: LabeledExpand(exporter_secret, "sec", exporter_context, L)
template <class HK>
CIRCL_HD void export_item(const ExportArgs &a, size_t i) {
    uint32_t prk[HK::OUT / 4];
    for (int j = 0; j < HK::OUT / 4; j++) prk[j] = a.ctx[i * a.ctx_stride_words + CTX_HEAD_WORDS + j];
    const uint8_t *exp;
    const uint64_t exp_len = range_of(exp, a.exp, a.exp_off, i);
    hkdf::labeled_expand_stream<HK, EXPORT_WAVES>(a.out + i * (size_t)a.L, a.L, prk, SuiteId{a.kem, a.kdf, a.aead}, "sec", exp, exp_len, 0xff);
}

template <class C, class HK, bool SENDER>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(C::WAVES, C::WAVES))) void setup_kernel(const SetupArgs a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    setup_item<C, HK, SENDER>(a, i);
}

template <bool SEAL>
static __global__ __launch_bounds__(64) void aead_kernel(const AeadArgs a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    aead_item<SEAL>(a, i);
}

template <class HK>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(EXPORT_WAVES, EXPORT_WAVES))) void export_kernel(const ExportArgs a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    export_item<HK>(a, i);
}

}  // namespace hpke
}  // namespace circl

#undef CIRCL_HPKE_CALL
