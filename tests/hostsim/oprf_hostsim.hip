// tests/hostsim/oprf_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/ristretto255_dev.h and oprf_group_kernels.h on the CPU (their host instantiation), so that the CPU-only test tier can
// check the very source the ristretto255 / OPRF kernels are built from against the checker tests/oprf.py.
// Nothing here is linked into libcirclhip.so.
//
// With -DOPRF_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: ragged batches whose blobs are heap blocks of exactly
// their size go through every item function, and finalize(evaluate(blind(x))) must equal full_evaluate(x).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

// Only the host side of this file is ever run, and it is compiled host-only.  There the device's forced inlining buys nothing and
// costs minutes of compile time (every field product inlined into every caller), so the lane-local functions are plain inline here.
#define CIRCL_HD __host__ __device__ inline

#include "oprf_group_kernels.h"

using namespace circl;
using ed25519::Ge;
using x25519::Fe;

extern "C" {

// SQRT_RATIO_M1 on canonical words: the root's words and was_square
int hs_sqrt_ratio_m1(uint32_t *root, const uint32_t *u, const uint32_t *v) {
    Fe r;
    const bool sq = r255::sqrt_ratio_m1(r, x25519::fe_from_words(u), x25519::fe_from_words(v));
    x25519::fe_to_words(root, r);
    return sq;
}

// out = encode(decode(in)) (computed whatever the verdict); returns decode's verdict
int hs_decode_encode(uint32_t *out, const uint32_t *in) {
    Ge p;
    const uint32_t good = r255::r255_decode(p, in);
    r255::r255_encode(out, p);
    return (int)good;
}

int hs_equal_identity(const uint32_t *enc) { return r255::r255_equal_identity(enc); }

void hs_map(uint32_t *out, const uint32_t *t) { r255::r255_encode(out, r255::r255_map(t)); }

void hs_from_uniform(uint32_t *out, const uint32_t *u) { r255::r255_encode(out, r255::r255_from_uniform(u)); }

void hs_xmd64(uint32_t *out, const uint8_t *pre, uint32_t pre_len, const uint8_t *body, uint64_t body_len, const uint8_t *suf, uint32_t suf_len,
              const uint8_t *dst, uint32_t dst_len) {
    hkdf::xmd<hkdf::Sha512, oprf::WAVES>(out, 64, pre, pre_len, body, body_len, suf, suf_len, dst, dst_len);
}

void hs_sc_mul(uint32_t *out, const uint32_t *a, const uint32_t *b) { r255::sc_mul(out, a, b); }
void hs_sc_inv(uint32_t *out, const uint32_t *x) { r255::sc_inv(out, x); }

// out = encode(k decode(elem)) through the constant-time multiplication; returns decode's verdict
int hs_mul(uint32_t *out, const uint32_t *k, const uint32_t *elem) {
    Ge p;
    const uint32_t good = r255::r255_decode(p, elem);
    r255::r255_encode(out, r255::r255_mul(k, p));
    return (int)good;
}

void hs_base(uint32_t *out, const uint32_t *k) { r255::r255_encode(out, r255::r255_base(k)); }

void hs_item(int op, const oprf::Args *a, uint64_t i) {
    switch (op) {
        case oprf::kHashToGroup: oprf::Item<oprf::R255, oprf::kHashToGroup, oprf::WAVES>::run(*a, i); break;
        case oprf::kHashToScalar: oprf::Item<oprf::R255, oprf::kHashToScalar, oprf::WAVES>::run(*a, i); break;
        case oprf::kScalarMult: oprf::Item<oprf::R255, oprf::kScalarMult, oprf::WAVES>::run(*a, i); break;
        case oprf::kDeriveKeyPair: oprf::Item<oprf::R255, oprf::kDeriveKeyPair, oprf::WAVES>::run(*a, i); break;
        case oprf::kBlind: oprf::Item<oprf::R255, oprf::kBlind, oprf::WAVES>::run(*a, i); break;
        case oprf::kEvaluate: oprf::Item<oprf::R255, oprf::kEvaluate, oprf::WAVES>::run(*a, i); break;
        case oprf::kFinalize: oprf::Item<oprf::R255, oprf::kFinalize, oprf::WAVES>::run(*a, i); break;
        case oprf::kFullEvaluate: oprf::Item<oprf::R255, oprf::kFullEvaluate, oprf::WAVES>::run(*a, i); break;
    }
}

}  // extern "C"

#ifdef OPRF_HOSTSIM_MAIN
#include <cstdio>
#include <cstdlib>
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

// exact-size rows of 32-bit words
struct Rows {
    uint32_t *w;
    explicit Rows(size_t words) : w(static_cast<uint32_t *>(calloc(words ? words : 1, 4))) {}
    ~Rows() { free(w); }
    Rows(const Rows &) = delete;
    uint8_t *b() { return reinterpret_cast<uint8_t *>(w); }
};

void set_dst(oprf::Args &a, const char *label, int mode) {
    const char tail[] = "-ristretto255-SHA512";
    size_t at = 0;
    for (const char *s = label; *s; s++) a.dst[at++] = (uint8_t)*s;
    for (const char *s = "OPRFV1-"; *s; s++) a.dst[at++] = (uint8_t)*s;
    a.dst[at++] = (uint8_t)mode;
    for (const char *s = tail; *s; s++) a.dst[at++] = (uint8_t)*s;
    a.dst_len = (uint32_t)at;
}

int fail(const char *what) {
    printf("FAIL %s\n", what);
    return 1;
}

int run(int mode) {
    const size_t n = 20;
    // lengths on both sides of the SHA-512 padding edges of the xmd and the Finalize message
    Rag in(n, [](size_t i) { static const size_t L[] = {0, 1, 67, 68, 83, 84, 85, 195, 196, 1000}; return L[i % 10]; }, 11 + mode);
    Rag info(n, [](size_t i) { return i * 3; }, 5);
    Rows seeds(8 * n), sk(8 * n), pk(8 * n), blinds(8 * n), blinded(8 * n), evaluated(8 * n), out(16 * n), full(16 * n), unblinded(8 * n);
    std::vector<uint8_t> ok(n);
    uint32_t seed = 99;
    for (size_t j = 0; j < 8 * n; j++) seeds.w[j] = seed = seed * 1664525u + 1013904223u;
    oprf::Args a = {};
    a.n = n;
    a.ok = ok.data();
    // keys
    a.blob = info.blob; a.off = info.off.data(); a.seeds = seeds.w; a.out = sk.b(); a.out2 = pk.b();
    set_dst(a, "DeriveKeyPair", mode);
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kDeriveKeyPair, &a, i); if (!ok[i]) return fail("derive_keypair refused an item"); }
    // blinds: any non-zero canonical scalars; the keys serve
    for (size_t j = 0; j < 8 * n; j++) blinds.w[j] = sk.w[8 * ((j / 8 + 1) % n) + j % 8];
    a.blob = in.blob; a.off = in.off.data(); a.scalars = blinds.w; a.scalar_stride = 8; a.elems = nullptr; a.out = blinded.b(); a.out2 = nullptr;
    set_dst(a, "HashToGroup-", mode);
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kBlind, &a, i); if (!ok[i]) return fail("blind refused an item"); }
    // evaluate under the shared key sk[0], finalize, and the same in one step
    a.blob = nullptr; a.off = nullptr; a.scalars = sk.w; a.scalar_stride = 0; a.elems = blinded.b(); a.out = evaluated.b();
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kEvaluate, &a, i); if (!ok[i]) return fail("evaluate refused an item"); }
    a.blob = in.blob; a.off = in.off.data(); a.scalars = blinds.w; a.scalar_stride = 8; a.elems = evaluated.b(); a.out = out.b();
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kFinalize, &a, i); if (!ok[i]) return fail("finalize refused an item"); }
    a.scalars = sk.w; a.scalar_stride = 0; a.elems = nullptr; a.out = full.b();
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kFullEvaluate, &a, i); if (!ok[i]) return fail("full_evaluate refused an item"); }
    if (memcmp(out.w, full.w, 64 * n)) return fail("finalize(evaluate(blind(x))) != full_evaluate(x)");
    // scalar_mult by the inverse undoes a blinding: blind^-1 (blind P) = P = hash_to_group(x)
    a.blob = nullptr; a.off = nullptr; a.scalars = blinds.w; a.scalar_stride = 8; a.elems = blinded.b(); a.out = unblinded.b(); a.flags = 1;
    for (size_t i = 0; i < n; i++) { hs_item(oprf::kScalarMult, &a, i); if (!ok[i]) return fail("scalar_mult refused an item"); }
    a.flags = 0; a.blob = in.blob; a.off = in.off.data(); a.out = evaluated.b();
    for (size_t i = 0; i < n; i++) hs_item(oprf::kHashToGroup, &a, i);
    if (memcmp(unblinded.w, evaluated.w, 32 * n)) return fail("blind^-1 (blind P) != P");
    for (size_t i = 0; i < n; i++) hs_item(oprf::kHashToScalar, &a, i);
    // failure masks: a zero blind, an element that does not decode
    memset(blinds.w, 0, 32);
    blinded.w[8] = 1;  // s = ...1: negative
    a.scalars = blinds.w; a.out = unblinded.b();
    hs_item(oprf::kBlind, &a, 0);
    a.scalars = sk.w; a.scalar_stride = 0; a.elems = blinded.b();
    hs_item(oprf::kEvaluate, &a, 1);
    for (int j = 0; j < 16; j++)
        if (unblinded.w[j]) return fail("a failed item's row is not zero");
    if (ok[0] || ok[1]) return fail("a bad blind or element passed");
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    for (int mode = 0; mode < 3; mode++) bad |= run(mode);
    // the byte-ragged hash at every length, on exact-size blocks and with tags of 1, 40 and 255 bytes
    for (uint32_t dl : {1u, 40u, 255u})
        for (size_t len = 0; len <= 300; len++) {
            uint8_t *m = static_cast<uint8_t *>(malloc(len ? len : 1)), *d = static_cast<uint8_t *>(malloc(dl));
            memset(m, (int)len, len);
            memset(d, 0x44, dl);
            uint32_t out[16];
            hs_xmd64(out, m, (uint32_t)(len / 3), m + len / 3, len - len / 3, nullptr, 0, d, dl);
            free(m);
            free(d);
        }
    puts(bad ? "oprf_hostsim: FAILED" : "oprf_hostsim: ok");
    return bad;
}
#endif
