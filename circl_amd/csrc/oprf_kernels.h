// oprf_kernels.h -- batch ristretto255 group operations (group/ristretto255.go) and the proof-free part of OPRF (RFC 9497, suite
// ristretto255-SHA512; oprf/keys.go, oprf/client.go, oprf/server.go) on ristretto255_dev.h: one item per lane, one launch per call,
// no workspace.
//
// One item function per public operation (item<OP, WV>), one kernel per item function.  The expand_message_xmd and the Finalize
// hash are functions of their own (xmd64, finalize_hash), so that the field loops of the multiplication keep their register
// allocation and what a hash holds does not live across them; each is instantiated for the occupancy class of the kernels (WAVES).
// A hashed point, an evaluated element before it is hashed, a blind's inverse: none of them reaches memory.
//
// Failure is a mask: ok[i] = 0 and every output row of item i is zero.  The verdicts are computed without a branch on a secret;
// only lengths (public) steer loops.  Secrets a lane held are zeroed before it returns.
#pragma once
#include <hip/hip_runtime.h>

#include "ristretto255_dev.h"

namespace circl {
namespace oprf {

using ed25519::Ge;

constexpr int WAVES = 2;  // the Ed25519 kernels' class: a point, a cached addend and a product's column sums in 256 registers
constexpr uint64_t kMaxInputBytes = 0xffff;  // RFC 9497: inputs and infos carry a two-byte length

enum Op : int { kHashToGroup = 0, kHashToScalar, kScalarMult, kDeriveKeyPair, kBlind, kEvaluate, kFinalize, kFullEvaluate, kOps };

struct Args {
    const uint8_t *blob;       // the ragged argument (messages, infos, inputs); nullptr: every item's is empty
    const uint64_t *off;
    const uint32_t *scalars;   // rows of 8 words, scalar_stride words apart (0: one row for the batch): scalars, keys, blinds
    size_t scalar_stride;
    const uint32_t *elems;     // rows of 8 words: elements, blinded / evaluated elements, seeds; nullptr (kScalarMult): the generator
    uint32_t *out;             // rows of 8 words; 16 for kFinalize / kFullEvaluate
    uint32_t *out2;            // kDeriveKeyPair: the public keys
    uint8_t *ok;               // may be nullptr
    uint32_t flags;            // kScalarMult: bit 0 = by the scalar's inverse
    uint32_t dst_len;
    size_t n;
    uint8_t dst[256];          // the domain separation tag of the launch's hash
};

CIRCL_HD uint64_t item_range(const uint8_t *&p, const Args &a, size_t i) {
    if (!a.blob || !a.off) {
        p = nullptr;
        return 0;
    }
    p = a.blob + a.off[i];
    return a.off[i + 1] - a.off[i];
}
CIRCL_HD void load8(uint32_t w[8], const uint32_t *p) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = p[j];
}
template <int N>
CIRCL_HD void store_masked(uint32_t *p, const uint32_t *w, uint32_t good) {
    const uint32_t mask = 0u - good;
#pragma unroll
    for (int j = 0; j < N; j++) p[j] = w[j] & mask;
}
template <int N>
CIRCL_HD void wipe(uint32_t *w) {
#pragma unroll
    for (int j = 0; j < N; j++) w[j] = 0;
}
CIRCL_HD void wipe(Ge &p) { p = ed25519::ge_identity(); }
// 1 for a scalar a key or a blind may be: canonical and not zero
CIRCL_HD uint32_t secret_scalar_ok(const uint32_t k[8]) { return ed25519::sc_is_canonical(k) & (r255::sc_is_zero(k) ? 0u : 1u); }

// oprf/client.go Finalize / server.go FullEvaluate: SHA-512(I2OSP(len, 2) || input || I2OSP(32, 2) || element || "Finalize")
template <int WV>
CIRCL_HKDF_STREAM_CALL(WV) void finalize_hash(uint32_t *out, const uint8_t *input, uint64_t len, const uint32_t *element) {
    hkdf::Stream<hkdf::Sha512, WV> st;
    st.init();
    st.put((uint8_t)(len >> 8));
    st.put((uint8_t)len);
    st.put(input, len);
    st.put((uint8_t)0);
    st.put((uint8_t)32);
    st.put(reinterpret_cast<const uint8_t *>(element), 32);
    const char tag[] = "Finalize";
    for (int j = 0; j < 8; j++) st.put((uint8_t)tag[j]);
    st.finish(out);
}

template <int OP, int WV>
CIRCL_HD void item(const Args &a, size_t i);

// group.Ristretto255.HashToElement(msg, dst)
template <>
CIRCL_HD void item<kHashToGroup, WAVES>(const Args &a, size_t i) {
    const uint8_t *m;
    const uint64_t len = item_range(m, a, i);
    uint32_t u[16], enc[8];
    r255::xmd64<WAVES>(u, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
    r255::r255_encode(enc, r255::r255_from_uniform(u));
    store_masked<8>(a.out + 8 * i, enc, 1);
}

// group.Ristretto255.HashToScalar(msg, dst)
template <>
CIRCL_HD void item<kHashToScalar, WAVES>(const Args &a, size_t i) {
    const uint8_t *m;
    const uint64_t len = item_range(m, a, i);
    uint32_t u[16], s[8];
    r255::xmd64<WAVES>(u, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
    r255::sc_from_uniform(s, u);
    store_masked<8>(a.out + 8 * i, s, 1);
}

// Element.Mul / Element.MulGen, optionally by the scalar's inverse: the scalar below L, the element any valid one (the identity too)
template <>
CIRCL_HD void item<kScalarMult, WAVES>(const Args &a, size_t i) {
    uint32_t k[8], kinv[8], enc[8];
    load8(k, a.scalars + i * a.scalar_stride);
    uint32_t good = ed25519::sc_is_canonical(k);
    if (a.flags & 1u) {  // (a launch-wide flag)
        good &= r255::sc_is_zero(k) ? 0u : 1u;
        r255::sc_inv(kinv, k);
        load8(k, kinv);
    }
    Ge p;
    if (a.elems) {
        uint32_t e[8];
        load8(e, a.elems + 8 * i);
        good &= r255::r255_decode(p, e);
        p = r255::r255_mul(k, p);
    } else {
        p = r255::r255_base(k);
    }
    r255::r255_encode(enc, p);
    store_masked<8>(a.out + 8 * i, enc, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<8>(k);
    wipe<8>(kinv);
    wipe(p);
}

// oprf/keys.go DeriveKey: sk = HashToScalar(seed || I2OSP(len(info), 2) || info || counter, "DeriveKeyPair" || ctx) for the first
// counter in 0..255 that gives a non-zero scalar, pk = sk B.  The loop ends on "the scalar is not zero": a scalar that the loop
// discards is never a key, and that a candidate was zero (probability 2^-252 each) says nothing about the one that is kept.
template <>
CIRCL_HD void item<kDeriveKeyPair, WAVES>(const Args &a, size_t i) {
    const uint8_t *info;
    const uint64_t info_len = item_range(info, a, i);
    const bool fits = info_len <= kMaxInputBytes;
    uint32_t pre[9], u[16], sk[8], pk[8];
    load8(pre, a.elems + 8 * i);
    pre[8] = (uint32_t)((info_len >> 8) & 0xff) | (uint32_t)(info_len & 0xff) << 8;
    uint32_t good = 0;
    wipe<8>(sk);
    for (uint32_t counter = 0; counter < 256 && !good; counter++) {
        const uint8_t c = (uint8_t)counter;
        r255::xmd64<WAVES>(u, reinterpret_cast<const uint8_t *>(pre), 34, info, fits ? info_len : 0, &c, 1, a.dst, a.dst_len);
        r255::sc_from_uniform(sk, u);
        good = r255::sc_is_zero(sk) ? 0u : 1u;
    }
    good &= fits ? 1u : 0u;
    Ge p = r255::r255_base(sk);
    r255::r255_encode(pk, p);
    store_masked<8>(a.out + 8 * i, sk, good);
    store_masked<8>(a.out2 + 8 * i, pk, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<9>(pre);
    wipe<16>(u);
    wipe<8>(sk);
    wipe(p);
}

// oprf/client.go DeterministicBlind: blinded = blind HashToGroup(input)
template <>
CIRCL_HD void item<kBlind, WAVES>(const Args &a, size_t i) {
    const uint8_t *m;
    const uint64_t len = item_range(m, a, i);
    const bool fits = len <= kMaxInputBytes;
    uint32_t u[16], k[8], enc[8];
    load8(k, a.scalars + i * a.scalar_stride);
    uint32_t good = secret_scalar_ok(k) & (fits ? 1u : 0u);
    r255::xmd64<WAVES>(u, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
    Ge p = r255::r255_from_uniform(u);
    p = r255::r255_mul(k, p);
    r255::r255_encode(enc, p);
    // blind != 0 and the group has prime order: the blinded element is the identity exactly where the hashed point is
    good &= r255::r255_equal_identity(enc) ? 0u : 1u;
    store_masked<8>(a.out + 8 * i, enc, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<16>(u);
    wipe<8>(k);
    wipe(p);
}

// oprf/server.go Server.Evaluate (base mode): evaluated = sk blinded
template <>
CIRCL_HD void item<kEvaluate, WAVES>(const Args &a, size_t i) {
    uint32_t k[8], e[8], enc[8];
    load8(k, a.scalars + i * a.scalar_stride);
    load8(e, a.elems + 8 * i);
    Ge p;
    uint32_t good = secret_scalar_ok(k) & r255::r255_decode(p, e) & (r255::r255_equal_identity(e) ? 0u : 1u);
    p = r255::r255_mul(k, p);
    r255::r255_encode(enc, p);
    store_masked<8>(a.out + 8 * i, enc, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<8>(k);
    wipe(p);
}

// oprf/client.go Client.Finalize (base mode): output = Hash(input, blind^-1 evaluated)
template <>
CIRCL_HD void item<kFinalize, WAVES>(const Args &a, size_t i) {
    const uint8_t *m;
    const uint64_t len = item_range(m, a, i);
    const bool fits = len <= kMaxInputBytes;
    uint32_t k[8], kinv[8], e[8], enc[8], h[16];
    load8(k, a.scalars + i * a.scalar_stride);
    load8(e, a.elems + 8 * i);
    Ge p;
    uint32_t good = secret_scalar_ok(k) & r255::r255_decode(p, e) & (r255::r255_equal_identity(e) ? 0u : 1u) & (fits ? 1u : 0u);
    r255::sc_inv(kinv, k);
    p = r255::r255_mul(kinv, p);
    r255::r255_encode(enc, p);
    finalize_hash<WAVES>(h, m, fits ? len : 0, enc);
    store_masked<16>(a.out + 16 * i, h, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<8>(k);
    wipe<8>(kinv);
    wipe<8>(enc);
    wipe<16>(h);
    wipe(p);
}

// oprf/server.go Server.FullEvaluate / VerifiableServer.FullEvaluate: output = Hash(input, sk HashToGroup(input))
template <>
CIRCL_HD void item<kFullEvaluate, WAVES>(const Args &a, size_t i) {
    const uint8_t *m;
    const uint64_t len = item_range(m, a, i);
    const bool fits = len <= kMaxInputBytes;
    uint32_t u[16], k[8], enc[8], h[16];
    load8(k, a.scalars + i * a.scalar_stride);
    uint32_t good = secret_scalar_ok(k) & (fits ? 1u : 0u);
    r255::xmd64<WAVES>(u, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
    Ge p = r255::r255_from_uniform(u);
    p = r255::r255_mul(k, p);
    r255::r255_encode(enc, p);
    good &= r255::r255_equal_identity(enc) ? 0u : 1u;  // as in kBlind: the hashed point was the identity
    finalize_hash<WAVES>(h, m, fits ? len : 0, enc);
    store_masked<16>(a.out + 16 * i, h, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<16>(u);
    wipe<8>(k);
    wipe<8>(enc);
    wipe<16>(h);
    wipe(p);
}

template <int OP>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    item<OP, WAVES>(a, i);
}

}  // namespace oprf
}  // namespace circl
