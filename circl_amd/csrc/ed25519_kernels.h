// ed25519_kernels.h -- batch Ed25519 (sign/ed25519: NewKeyFromSeed, Sign, Verify) and batch SHA-512, one item per lane.
// A wavefront is 64 independent items: no LDS, no cross-lane traffic.  Key generation and signing are one comb each (the
// comb of X25519 KeyGen) around two / four SHA-512 blocks and the scalar arithmetic; verification is one SHA-512 of
// R || A || M, a point decompression and a joint double-scalar multiplication whose multiples of -A sit in the workspace.
// Messages are the project's ragged blob: item i's bytes are msg_blob[msg_off[i] .. msg_off[i + 1]).
#pragma once
#include <hip/hip_runtime.h>

#include "ed25519_dev.h"
#include "keccak_dev.h"

namespace circl {
namespace ed25519 {

// NewKeyFromSeed (ed25519.go:206-223): h = SHA-512(seed), s = clamp(h[0..32)), A = enc(s B); pk = A, sk = seed || A.
// pk or sk may be nullptr.
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed25519_keygen_kernel(
    const uint32_t *__restrict__ seed, uint32_t *__restrict__ pk, uint32_t *__restrict__ sk, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t sd[8], h[16], a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sd[j] = seed[i * 8 + j];
    sha512::hash<8>(h, sd, nullptr, 0);
    clamp(h);
    ge_encode(a, ge_base(h));
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (pk) pk[i * 8 + j] = a[j];
        if (sk) {
            sk[i * 16 + j] = sd[j];
            sk[i * 16 + 8 + j] = a[j];
        }
    }
}

// Sign, pure Ed25519 (ed25519.go signAll :225-284 with an empty context and no pre-hash):
//   h = SHA-512(sk[0..32)), s = clamp(h[0..32)), prefix = h[32..64); r = SHA-512(prefix || M) mod L; R = enc(r B);
//   k = SHA-512(R || sk[32..64) || M) mod L -- the stored public half, as it is; S = (r + k s) mod L; sig = R || S.
// s is derived twice (before the nonce and after the comb) rather than kept alive across the comb.
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed25519_sign_kernel(
    const uint32_t *__restrict__ sk, const uint8_t *__restrict__ msg_blob, const uint64_t *__restrict__ msg_off,
    uint32_t *__restrict__ sig, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
    const uint8_t *msg = msg_blob ? msg_blob + mo : nullptr;
    uint32_t h[16], r[8], rw[8];
    {
        uint32_t sd[8], prefix[8], rr[16];
#pragma unroll
        for (int j = 0; j < 8; j++) sd[j] = sk[i * 16 + j];
        sha512::hash<8>(h, sd, nullptr, 0);
#pragma unroll
        for (int j = 0; j < 8; j++) prefix[j] = h[8 + j];
        sha512::hash<8>(rr, prefix, msg, ml);
        sc_reduce(r, rr);
    }
    ge_encode(rw, ge_base(r));
    uint32_t k[8];
    {
        uint32_t head[16], kk[16];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            head[j] = rw[j];
            head[8 + j] = sk[i * 16 + 8 + j];
        }
        sha512::hash<16>(kk, head, msg, ml);
        sc_reduce(k, kk);
    }
    {
        uint32_t sd[8], s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) sd[j] = sk[i * 16 + j];
        sha512::hash<8>(h, sd, nullptr, 0);
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = h[j];
        clamp(s);
        uint32_t S[8];
        sc_muladd(S, k, s, r);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            sig[i * 16 + j] = rw[j];
            sig[i * 16 + 8 + j] = S[j];
        }
    }
}

// Verify (ed25519.go verify :329-366, cofactorless): ok = S < L, A decodes, and enc([S]B - [k]A) equals the 32 bytes of R,
// k = SHA-512(R || pk || M) mod L over the pk bytes as given.  R is never decoded.  Two launches over the workspace
// ws (kVerifyWsBytes per item, all of it public): the first decodes A, writes the multiples of -A, k and the verdict so far;
// the second runs the double-scalar multiplication with nothing else alive (no spills at two waves per SIMD).
// ws layout, word-major across items: [0, 320) the table of ed25519_dev.h, [320, 328) k, 328 the verdict so far.
constexpr size_t kVerifyWords = 8 * 40 + 8 + 1;
constexpr size_t kVerifyWsBytes = kVerifyWords * 4;

static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed25519_verify_prep_kernel(
    const uint32_t *__restrict__ pk, const uint32_t *__restrict__ sig, const uint8_t *__restrict__ msg_blob,
    const uint64_t *__restrict__ msg_off, uint32_t *__restrict__ ws, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
    const uint8_t *msg = msg_blob ? msg_blob + mo : nullptr;
    uint32_t head[16], s[8], kk[16], k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        head[j] = sig[i * 16 + j];
        head[8 + j] = pk[i * 8 + j];
        s[j] = sig[i * 16 + 8 + j];
    }
    uint32_t good = sc_is_canonical(s);
    Ge a;
    good &= ge_decode(a, head + 8);
    a.X = fe_carry(fe_neg(a.X));  // -A
    a.T = fe_carry(fe_neg(a.T));
    table_build(ws, n, i, a);
    sha512::hash<16>(kk, head, msg, ml);
    sc_reduce(k, kk);
#pragma unroll
    for (int j = 0; j < 8; j++) ws[(320 + j) * n + i] = k[j];
    ws[328 * n + i] = good;
}

static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed25519_verify_kernel(
    const uint32_t *__restrict__ sig, uint8_t *__restrict__ ok, const uint32_t *__restrict__ ws, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8], k[8], rw[8];
    const uint32_t good = ws[328 * n + i];
#pragma unroll
    for (int j = 0; j < 8; j++) {  // a rejected item runs with S = 0: an S >= L would have top digits past the comb's row
        s[j] = good ? sig[i * 16 + 8 + j] : 0u;
        k[j] = ws[(320 + j) * n + i];
    }
    ge_encode(rw, double_scalar_mult(s, k, ws, n, i));
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d |= rw[j] ^ sig[i * 16 + j];
    ok[i] = (uint8_t)(good && d == 0 ? 1 : 0);
}

// out[i] = SHA-512(msg_i), 64 bytes
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void sha512_kernel(const uint8_t *__restrict__ msg_blob, const uint64_t *__restrict__ msg_off,
                                                           uint32_t *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
    uint32_t h[16];
    sha512::hash<0>(h, nullptr, msg_blob ? msg_blob + mo : nullptr, ml);
#pragma unroll
    for (int j = 0; j < 16; j++) out[i * 16 + j] = h[j];
}

// Ed25519-Dilithium2 key generation (sign/eddilithium2/eddilithium.go NewKeyFromSeed): SHAKE256(seed) -> 32 bytes for the
// Dilithium2 seed (seed_d), then 32 for the Ed25519 seed (seed_e).  One absorb of 32 bytes, one permutation, 64 bytes out.
static __global__ __launch_bounds__(64) void eddilithium2_seed_kernel(const uint32_t *__restrict__ seed, uint32_t *__restrict__ seed_d,
                                                                      uint32_t *__restrict__ seed_e, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    KeccakState st;
#pragma unroll
    for (int j = 0; j < 25; j++) st.lo[j] = st.hi[j] = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st.lo[j] = seed[i * 8 + 2 * j];
        st.hi[j] = seed[i * 8 + 2 * j + 1];
    }
    st.lo[4] ^= kDsShake;          // byte 32: the SHAKE domain bits and the first pad bit
    st.hi[16] ^= 0x80000000u;      // byte 135: the last pad bit of the 136-byte rate
    keccak_f1600(st);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        seed_d[i * 8 + 2 * j] = st.lo[j];
        seed_d[i * 8 + 2 * j + 1] = st.hi[j];
        seed_e[i * 8 + 2 * j] = st.lo[4 + j];
        seed_e[i * 8 + 2 * j + 1] = st.hi[4 + j];
    }
}

}  // namespace ed25519
}  // namespace circl
