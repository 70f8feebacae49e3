// dhkem_kernels.h -- batch HPKE DHKEM (RFC 9180 section 4.1; hpke/kembase.go, hpke/xkem.go) over X25519 with HKDF-SHA256
// (KEM id 0x20) and X448 with HKDF-SHA512 (0x21): one item per lane, one launch per operation, no workspace.
//
// An operation is one to four scalar multiplications (the fixed-base comb where the point is the base point, the Montgomery
// ladder otherwise) with a few hash compressions between them (hkdf_dev.h): 17 SHA-256 compressions, ~6 x 10^4 instructions with
// the message building, against ~5 x 10^5 integer instructions of comb plus ladder for an X25519 encapsulation.  So an operation
// is ONE fused kernel, in which the ephemeral private key, the Diffie-Hellman outputs and the HKDF pseudorandom keys stay in the
// lane (registers, and the lane's own scratch around the calls below) and never reach memory the caller can see -- as Ed25519
// KeyGen and Sign keep theirs (ed25519_kernels.h).  Public rows that are needed again after a scalar multiplication (pkR, enc, pkS
// for kemCtx) are read again from global memory.
//
// The operations are __host__ __device__ functions on row pointers (op_*), which the kernels below wrap and which
// tests/hostsim/hpke_hostsim.hip runs on the CPU.  Failure (a low-order point, which x25519 / x448 Shared reject) is a mask, not a
// branch: ok = 0 and every output row of the item is zero.
#pragma once
#include <hip/hip_runtime.h>

#include "hkdf_dev.h"
#include "x25519_dev.h"
#include "x448_dev.h"

// A scalar multiplication is a function of its own, not inlined into the operation: it keeps the register allocation it has in
// the bare x25519 / x448 kernels, whatever the operation holds around it (what is live across the call is saved at the call, outside
// the loops), and an operation with two ladders carries one copy of the ladder.
#define CIRCL_DHKEM_CALL static __host__ __device__ __attribute__((noinline))

namespace circl {
namespace dhkem {

struct X25519 {
    static constexpr int KEM_ID = 0x20, W = 8, WAVES = 4;  // W: words of a key row; WAVES: the ladder's own allocation
    using H = hkdf::Sha256;
    CIRCL_DHKEM_CALL void base(uint32_t *out, const uint32_t *k) { x25519::base_mult(out, k); }
    CIRCL_DHKEM_CALL void shared(uint32_t *out, const uint32_t *k, const uint32_t *u) { x25519::scalar_mult<false>(out, k, u); }
    static CIRCL_HD uint32_t valid(const uint32_t *u) {  // key.go:24-31 on the point with bit 255 cleared
        uint32_t m[8];
#pragma unroll
        for (int j = 0; j < 8; j++) m[j] = u[j];
        m[7] &= 0x7fffffffu;
        return x25519::valid_public(m);
    }
};

struct X448 {
    static constexpr int KEM_ID = 0x21, W = 14, WAVES = 2;
    using H = hkdf::Sha512;
    CIRCL_DHKEM_CALL void base(uint32_t *out, const uint32_t *k) { x448::base_mult_comb(out, k); }
    CIRCL_DHKEM_CALL void shared(uint32_t *out, const uint32_t *k, const uint32_t *u) { x448::scalar_mult<false>(out, k, u); }
    static CIRCL_HD uint32_t valid(const uint32_t *u) { return x448::valid_public(u); }
};

template <class C>
CIRCL_HD void load_row(uint32_t *r, const uint32_t *p) {
#pragma unroll
    for (int j = 0; j < C::W; j++) r[j] = p[j];
}

// xkem.go:55-71 DeriveKeyPair: sk = LabeledExpand(LabeledExtract("", "dkp_prk", ikm), "sk", "", Nsk), unclamped
template <class C>
CIRCL_HD void derive_sk(uint32_t *sk, const uint32_t *ikm) {
    uint32_t prk[C::H::OUT / 4];
    hkdf::labeled_extract<typename C::H, C::KEM_ID, C::W>(prk, "dkp_prk", ikm);
    hkdf::labeled_expand<typename C::H, C::KEM_ID, 4 * C::W, 0>(sk, prk, "sk", nullptr);
}

// kembase.go:42-50 extractExpand: ss = LabeledExpand(LabeledExtract("", "eae_prk", dh), "shared_secret", kemCtx, Nsecret);
// dh = NDH rows, kemCtx = NDH + 1 rows, ss = H::OUT bytes
template <class C, int NDH>
CIRCL_HD void extract_expand(uint32_t *ss, const uint32_t *dh, const uint32_t *ctx) {
    uint32_t prk[C::H::OUT / 4];
    hkdf::labeled_extract<typename C::H, C::KEM_ID, NDH * C::W>(prk, "eae_prk", dh);
    hkdf::labeled_expand<typename C::H, C::KEM_ID, C::H::OUT, (NDH + 1) * C::W>(ss, prk, "shared_secret", ctx);
}

template <class C>
CIRCL_HD void store_masked(uint32_t *p, const uint32_t *r, int words, uint32_t mask) {
#pragma unroll
    for (int j = 0; j < (C::H::OUT / 4 > C::W ? C::H::OUT / 4 : C::W); j++)
        if (j < words) p[j] = r[j] & mask;
}

// ---- the five operations on the rows of one item (4-byte aligned) ------------------------------------------------------------
template <class C>
CIRCL_HD void op_derive_keypair(const uint32_t *ikm, uint32_t *sk_out, uint32_t *pk_out) {
    uint32_t r[C::W], sk[C::W], pk[C::W];
    load_row<C>(r, ikm);
    derive_sk<C>(sk, r);
    store_masked<C>(sk_out, sk, C::W, 0xffffffffu);
    C::base(pk, sk);
    store_masked<C>(pk_out, pk, C::W, 0xffffffffu);
}

// kembase.go:120-131, 161-183: (pkE, skE) = DeriveKeyPair(ikmE); dh = DH(skE, pkR); kemCtx = enc || pkR
template <class C>
CIRCL_HD uint32_t op_encap(const uint32_t *pkR, const uint32_t *ikmE, uint32_t *enc, uint32_t *ss_out) {
    uint32_t r[C::W], sk[C::W], u[C::W], dh[C::W], ctx[2 * C::W], ss[C::H::OUT / 4];
    load_row<C>(r, ikmE);
    derive_sk<C>(sk, r);
    load_row<C>(u, pkR);
    const uint32_t good = C::valid(u), mask = 0u - good;
    C::shared(dh, sk, u);
    C::base(ctx, sk);
    store_masked<C>(enc, ctx, C::W, mask);
    load_row<C>(ctx + C::W, pkR);
    extract_expand<C, 1>(ss, dh, ctx);
    store_masked<C>(ss_out, ss, C::H::OUT / 4, mask);
    return good;
}

// kembase.go:185-192, 219-241: dh = DH(skR, pkE); kemCtx = enc || pkR, pkR = skR.Public() (computed here when it is not given)
template <class C>
CIRCL_HD uint32_t op_decap(const uint32_t *skR, const uint32_t *pkR, const uint32_t *enc, uint32_t *ss_out) {
    uint32_t sk[C::W], u[C::W], dh[C::W], ctx[2 * C::W], ss[C::H::OUT / 4];
    load_row<C>(sk, skR);
    load_row<C>(u, enc);
    const uint32_t good = C::valid(u), mask = 0u - good;
    C::shared(dh, sk, u);
    if (pkR) load_row<C>(ctx + C::W, pkR);
    else C::base(ctx + C::W, sk);
    load_row<C>(ctx, enc);
    extract_expand<C, 1>(ss, dh, ctx);
    store_masked<C>(ss_out, ss, C::H::OUT / 4, mask);
    return good;
}

// kembase.go:133-159: dh = DH(skE, pkR) || DH(skS, pkR); kemCtx = enc || pkR || pkS, pkS = skS.Public()
template <class C>
CIRCL_HD uint32_t op_auth_encap(const uint32_t *pkR, const uint32_t *skS, const uint32_t *pkS, const uint32_t *ikmE, uint32_t *enc, uint32_t *ss_out) {
    uint32_t r[C::W], sk[C::W], u[C::W], dh[2 * C::W], ctx[3 * C::W], ss[C::H::OUT / 4];
    load_row<C>(r, ikmE);
    derive_sk<C>(sk, r);
    load_row<C>(u, pkR);
    const uint32_t good = C::valid(u), mask = 0u - good;
    C::shared(dh, sk, u);
    C::base(ctx, sk);
    store_masked<C>(enc, ctx, C::W, mask);
    load_row<C>(sk, skS);
    load_row<C>(u, pkR);
    C::shared(dh + C::W, sk, u);
    if (pkS) load_row<C>(ctx + 2 * C::W, pkS);
    else C::base(ctx + 2 * C::W, sk);
    load_row<C>(ctx + C::W, pkR);
    extract_expand<C, 2>(ss, dh, ctx);
    store_masked<C>(ss_out, ss, C::H::OUT / 4, mask);
    return good;
}

// kembase.go:194-217: dh = DH(skR, pkE) || DH(skR, pkS); kemCtx = enc || pkR || pkS
template <class C>
CIRCL_HD uint32_t op_auth_decap(const uint32_t *skR, const uint32_t *pkR, const uint32_t *enc, const uint32_t *pkS, uint32_t *ss_out) {
    uint32_t sk[C::W], u[C::W], dh[2 * C::W], ctx[3 * C::W], ss[C::H::OUT / 4];
    load_row<C>(sk, skR);
    load_row<C>(u, enc);
    uint32_t good = C::valid(u);
    C::shared(dh, sk, u);
    load_row<C>(u, pkS);
    good &= C::valid(u);
    const uint32_t mask = 0u - good;
    C::shared(dh + C::W, sk, u);
    if (pkR) load_row<C>(ctx + C::W, pkR);
    else C::base(ctx + C::W, sk);
    load_row<C>(ctx, enc);
    load_row<C>(ctx + 2 * C::W, pkS);
    extract_expand<C, 2>(ss, dh, ctx);
    store_masked<C>(ss_out, ss, C::H::OUT / 4, mask);
    return good;
}

// ---- kernels: rows of C::W words (keys, enc) and C::H::OUT / 4 words (ss); ok may be nullptr --------------------------------
#define CIRCL_DHKEM_KERNEL template <class C> static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(C::WAVES, C::WAVES))) void

CIRCL_DHKEM_KERNEL derive_keypair_kernel(const uint32_t *__restrict__ ikm, uint32_t *__restrict__ sk, uint32_t *__restrict__ pk, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    op_derive_keypair<C>(ikm + i * C::W, sk + i * C::W, pk + i * C::W);
}

CIRCL_DHKEM_KERNEL encap_kernel(const uint32_t *__restrict__ pkR, const uint32_t *__restrict__ ikmE, uint32_t *__restrict__ enc, uint32_t *__restrict__ ss,
                                uint8_t *__restrict__ ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t good = op_encap<C>(pkR + i * C::W, ikmE + i * C::W, enc + i * C::W, ss + i * (C::H::OUT / 4));
    if (ok) ok[i] = (uint8_t)good;
}

CIRCL_DHKEM_KERNEL decap_kernel(const uint32_t *__restrict__ skR, const uint32_t *__restrict__ pkR, const uint32_t *__restrict__ enc, uint32_t *__restrict__ ss,
                                uint8_t *__restrict__ ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t good = op_decap<C>(skR + i * C::W, pkR ? pkR + i * C::W : nullptr, enc + i * C::W, ss + i * (C::H::OUT / 4));
    if (ok) ok[i] = (uint8_t)good;
}

CIRCL_DHKEM_KERNEL auth_encap_kernel(const uint32_t *__restrict__ pkR, const uint32_t *__restrict__ skS, const uint32_t *__restrict__ pkS,
                                     const uint32_t *__restrict__ ikmE, uint32_t *__restrict__ enc, uint32_t *__restrict__ ss, uint8_t *__restrict__ ok,
                                     size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t good =
        op_auth_encap<C>(pkR + i * C::W, skS + i * C::W, pkS ? pkS + i * C::W : nullptr, ikmE + i * C::W, enc + i * C::W, ss + i * (C::H::OUT / 4));
    if (ok) ok[i] = (uint8_t)good;
}

CIRCL_DHKEM_KERNEL auth_decap_kernel(const uint32_t *__restrict__ skR, const uint32_t *__restrict__ pkR, const uint32_t *__restrict__ enc,
                                     const uint32_t *__restrict__ pkS, uint32_t *__restrict__ ss, uint8_t *__restrict__ ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t good = op_auth_decap<C>(skR + i * C::W, pkR ? pkR + i * C::W : nullptr, enc + i * C::W, pkS + i * C::W, ss + i * (C::H::OUT / 4));
    if (ok) ok[i] = (uint8_t)good;
}

#undef CIRCL_DHKEM_KERNEL
#undef CIRCL_DHKEM_CALL

// out[i] = SHA-256(msg_i), 32 bytes (the twin of ed25519_kernels.h sha512_kernel)
static __global__ __launch_bounds__(64) void sha256_kernel(const uint8_t *__restrict__ msg_blob, const uint64_t *__restrict__ msg_off, uint32_t *__restrict__ out,
                                                           size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
    uint32_t h[8];
    sha256::hash<0>(h, nullptr, msg_blob ? msg_blob + mo : nullptr, ml);
#pragma unroll
    for (int j = 0; j < 8; j++) out[i * 8 + j] = h[j];
}

}  // namespace dhkem
}  // namespace circl
