// ed448_kernels.h -- batch Ed448 (sign/ed448: NewKeyFromSeed, Sign, Verify with a context), one item per lane.
// A wavefront is 64 independent items: no LDS, no cross-lane traffic.  Key generation and signing are one fixed-base
// multiplication each around two / four SHAKE256 calls and the scalar arithmetic; verification is one SHAKE256 of
// dom4 || R || A || M, a point decompression and a joint double-scalar multiplication whose multiples of -A sit in the workspace.
// Messages and contexts are the project's ragged blobs: item i's bytes are blob[off[i] .. off[i + 1]); a NULL context blob means
// every context is empty.  Rows of 57 and 114 bytes are not 4-byte aligned: they are read through bytes_word (aligned dwords that
// hold a byte of the row) and written byte by byte, so the row pointers need no alignment.
#pragma once
#include <hip/hip_runtime.h>

#include "ed448_dev.h"

namespace circl {
namespace ed448 {

// The item of this lane.  The lane id goes through an empty asm, so that what a later phase of a kernel derives from it (row
// pointers, offsets, lengths) is loaded again there instead of being kept in registers across the big loop in between.
__device__ __forceinline__ size_t item_index() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return (size_t)blockIdx.x * 64 + t;
}

// the context of item i: its length (0 when there is no context blob), and whether it is over ContextMaxSize
struct Ctx {
    const uint8_t *p;
    uint32_t len;
    bool too_long;
};
__device__ __forceinline__ Ctx ctx_of(const uint8_t *ctx_blob, const uint64_t *ctx_off, size_t i) {
    if (!ctx_blob || !ctx_off) return {nullptr, 0u, false};
    const uint64_t o = ctx_off[i], l = ctx_off[i + 1] - o;
    if (l > 255) return {nullptr, 0u, true};
    return {ctx_blob + o, (uint32_t)l, false};
}

// SHAKE256(seed, 114) -> the clamped scalar reduced mod l (s) and, if asked for, the prefix (57 bytes, fifteen words)
__device__ __forceinline__ void expand_seed(uint32_t s_clamped[14], uint32_t *prefix, const uint32_t (&seed)[15]) {
    uint32_t h[29];
    shake256_114<false, 15>(h, nullptr, 0, seed, 57, nullptr, 0);
#pragma unroll
    for (int j = 0; j < 14; j++) s_clamped[j] = h[j];
    clamp(s_clamped);
    if (prefix) {
#pragma unroll
        for (int j = 0; j < 15; j++) prefix[j] = (h[14 + j] >> 8) | (j < 14 ? h[15 + j] << 24 : 0u);
    }
}

// NewKeyFromSeed (ed448.go): h = SHAKE256(seed, 114), s = clamp(h[0..57)), A = enc([s]B); pk = A, sk = seed || A.
// pk or sk may be nullptr.
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed448_keygen_kernel(const uint8_t *__restrict__ seed, uint8_t *__restrict__ pk,
                                                                                                         uint8_t *__restrict__ sk, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t sd[15], s[14], sr[14], a[15];
    load_row(sd, seed + i * 57, 57);
    expand_seed(s, nullptr, sd);
    sc_reduce_small(sr, s);
    ge_encode(a, ge_base(sr));
    if (pk) store_row(pk + i * 57, a, 57);
    if (sk) {
        load_row(sd, seed + i * 57, 57);
        store_row(sk + i * 114, sd, 57);
        store_row(sk + i * 114 + 57, a, 57);
    }
}

// Sign, pure Ed448 (ed448.go signAll, no pre-hash): dom4 = "SigEd448" || 0x00 || len(ctx) || ctx;
//   h = SHAKE256(sk[0..57), 114), s = clamp(h[0..57)), prefix = h[57..114); r = SHAKE256(dom4 || prefix || M, 114) mod l;
//   R = enc([r]B); k = SHAKE256(dom4 || R || sk[57..114) || M, 114) mod l -- the stored public half, as it is;
//   S = (r + k s) mod l; sig = R || S (57 bytes, the last one 0).
// s is derived twice (before the nonce and after the fixed-base multiplication) rather than kept alive across it.
// The host refuses a context over 255 bytes before the launch; a device-resident batch that has one gets an all-zero signature.
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed448_sign_kernel(
    const uint8_t *__restrict__ sk, const uint8_t *__restrict__ msg_blob, const uint64_t *__restrict__ msg_off, const uint8_t *__restrict__ ctx_blob,
    const uint64_t *__restrict__ ctx_off, uint8_t *__restrict__ sig, size_t n) {
    if ((size_t)blockIdx.x * 64 + threadIdx.x >= n) return;
    uint32_t r[14], rw[15];
    {
        const size_t i = item_index();
        const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
        const Ctx cx = ctx_of(ctx_blob, ctx_off, i);
        uint32_t sd[15], s[14], prefix[15], rr[29];
        load_row(sd, sk + i * 114, 57);
        expand_seed(s, prefix, sd);
        shake256_114<true, 15>(rr, cx.p, cx.len, prefix, 57, msg_blob ? msg_blob + mo : nullptr, ml);
        sc_reduce(r, rr);
    }
    ge_encode(rw, ge_base(r));
    const size_t i = item_index();
    const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
    const uint8_t *msg = msg_blob ? msg_blob + mo : nullptr;
    const Ctx cx = ctx_of(ctx_blob, ctx_off, i);
    const uint8_t *row = sk + i * 114;
    uint32_t k[14];
    {
        uint32_t head[29], kk[29];
#pragma unroll
        for (int j = 0; j < 29; j++) head[j] = (j < 15 ? rw[j] : 0u) | (j >= 14 ? bytes_word(row + 57, 57, 4 * (j - 14) - 1) : 0u);
        shake256_114<true, 29>(kk, cx.p, cx.len, head, 114, msg, ml);
        sc_reduce(k, kk);
    }
    {
        uint32_t sd[15], s[14], S[15];
        load_row(sd, row, 57);
        expand_seed(s, nullptr, sd);
        sc_muladd(S, k, s, r);
        S[14] = 0u;
        if (cx.too_long) {
#pragma unroll
            for (int j = 0; j < 15; j++) rw[j] = S[j] = 0u;
        }
        store_row(sig + i * 114, rw, 57);
        store_row(sig + i * 114 + 57, S, 57);
    }
}

// Verify (ed448.go verify :294-339): ok = S < l with byte 56 zero, the context is at most 255 bytes, A decodes, and
// enc(CombinedMult(S, k, -A)) equals the 57 bytes of R, k = SHAKE256(dom4 || R || pk || M, 114) mod l over the pk bytes as given.
// R is never decoded.  Two launches over the workspace ws (kVerifyWsBytes per item, all of it public): the first hashes, writes
// the recoded S / 4 and k / 4 mod l, decodes A, writes the multiples of -A and the verdict so far; the second runs the joint
// multiplication with nothing else alive.  ws layout, word-major across items: [0, 512) the table of ed448_dev.h, [512, 540) the
// recoded scalars, 540 the verdict so far.
constexpr size_t kVerifyWords = kTableWords + kRecodedWords + 1;
constexpr size_t kVerifyWsBytes = kVerifyWords * 4;

static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed448_verify_prep_kernel(
    const uint8_t *__restrict__ pk, const uint8_t *__restrict__ sig, const uint8_t *__restrict__ msg_blob, const uint64_t *__restrict__ msg_off,
    const uint8_t *__restrict__ ctx_blob, const uint64_t *__restrict__ ctx_off, uint32_t *__restrict__ ws, size_t n) {
    if ((size_t)blockIdx.x * 64 + threadIdx.x >= n) return;
    uint32_t good;
    {
        const size_t i = item_index();
        const uint64_t mo = msg_off[i], ml = msg_off[i + 1] - mo;
        const Ctx cx = ctx_of(ctx_blob, ctx_off, i);
        uint32_t head[29], kk[29], k[14];
#pragma unroll
        for (int j = 0; j < 29; j++)
            head[j] = (j < 15 ? bytes_word(sig + i * 114, 57, 4 * j) : 0u) | (j >= 14 ? bytes_word(pk + i * 57, 57, 4 * (j - 14) - 1) : 0u);
        shake256_114<true, 29>(kk, cx.p, cx.len, head, 114, msg_blob ? msg_blob + mo : nullptr, ml);
        sc_reduce(k, kk);
        recode_store_div4(ws + kTableWords * n, n, i, 1, k);
        good = cx.too_long ? 0u : 1u;
    }
    {
        const size_t i = item_index();
        uint32_t s[15];
#pragma unroll
        for (int j = 0; j < 15; j++) s[j] = bytes_word(sig + i * 114, 114, 57 + 4 * j);
        good &= sc_is_canonical(s);
#pragma unroll
        for (int j = 0; j < 14; j++) s[j] = good ? s[j] : 0u;  // a rejected item runs with S = 0
        recode_store_div4(ws + kTableWords * n, n, i, 0, s);
    }
    const size_t i = item_index();
    uint32_t aw[15];
    load_row(aw, pk + i * 57, 57);
    Ge a;
    good &= ge_decode(a, aw);
    a.X = fe_neg(a.X);  // -A
    a.T = fe_neg(a.T);
    table_build(ws, n, i, a);
    ws[(kTableWords + kRecodedWords) * n + i] = good;
}

static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void ed448_verify_kernel(const uint8_t *__restrict__ sig, uint8_t *__restrict__ ok,
                                                                                                         const uint32_t *__restrict__ ws, size_t n) {
    if ((size_t)blockIdx.x * 64 + threadIdx.x >= n) return;
    uint32_t rw[15];
    {
        const size_t i = item_index();
        ge_encode(rw, combined_mult(ws + kTableWords * n, ws, n, i));
    }
    const size_t i = item_index();
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 15; j++) d |= rw[j] ^ bytes_word(sig + i * 114, 57, 4 * j);
    ok[i] = (uint8_t)(ws[(kTableWords + kRecodedWords) * n + i] && d == 0 ? 1 : 0);
}

// Ed448-Dilithium3 key generation (sign/eddilithium3/eddilithium.go NewKeyFromSeed): SHAKE256(seed57) -> 32 bytes for the
// Dilithium3 seed (seed_d, rows of 32), then 57 for the Ed448 seed (seed_e, rows of 57).  One block in, one block out.
static __global__ __launch_bounds__(64) void eddilithium3_seed_kernel(const uint8_t *__restrict__ seed, uint32_t *__restrict__ seed_d, uint8_t *__restrict__ seed_e,
                                                                      size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t sd[15], h[29], e[15];
    load_row(sd, seed + i * 57, 57);
    shake256_114<false, 15>(h, nullptr, 0, sd, 57, nullptr, 0);
#pragma unroll
    for (int j = 0; j < 8; j++) seed_d[i * 8 + j] = h[j];
#pragma unroll
    for (int j = 0; j < 15; j++) e[j] = h[8 + j];
    store_row(seed_e + i * 57, e, 57);
}

}  // namespace ed448
}  // namespace circl
