// x448_kernels.h -- batch X448 (dh/x448 KeyGen / Shared), one Montgomery ladder (Shared) or one fixed-base comb (KeyGen) per lane.
// A wavefront is 64 independent ladders: no LDS, no cross-lane traffic, 112 bytes in and 57 bytes out per item against 448 ladder
// steps of five products, four squarings and a small product in GF(2^448 - 2^224 - 1) -- pure VALU issue.
#pragma once
#include <hip/hip_runtime.h>

#include "x448_dev.h"

namespace circl {
namespace x448 {

// scalar, point, out: n rows of 56 bytes (4-byte aligned); ok[n] = 1 unless the point, reduced mod p, is 0, 1 or p - 1
// (key.go:22-30); BASE: point is ignored, the base point u = 5 is used (key.go:33-35), by the ladder or, with COMB, by the
// fixed-base comb of Ed448 (x448_dev.h base_mult_comb): the same bytes.
template <bool BASE, bool COMB = false>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void x448_kernel(const uint32_t *__restrict__ scalar, const uint32_t *__restrict__ point,
                                                                                                 uint32_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t k[14], u[14], r[14];
#pragma unroll
    for (int j = 0; j < 14; j++) {
        k[j] = scalar[i * 14 + j];
        u[j] = BASE ? 0u : point[i * 14 + j];
    }
    if (ok) ok[i] = BASE ? (uint8_t)1 : (uint8_t)valid_public(u);
    if (BASE && COMB) base_mult_comb(r, k);
    else scalar_mult<BASE>(r, k, u);
#pragma unroll
    for (int j = 0; j < 14; j++) out[i * 14 + j] = r[j];
}

// Both scalar multiplications of a hybrid encapsulation in ONE launch (as x25519_pair_kernel): workgroups [0, nb) compute the
// public keys X448(scalar_i, 5) -> out_base by the ladder or (COMB) the comb, workgroups [nb, 2 nb) the shared secrets
// X448(scalar_i, point_i) -> out_shared (+ ok) by the ladder.
template <bool COMB>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void x448_pair_kernel(const uint32_t *__restrict__ scalar, const uint32_t *__restrict__ point,
                                                                                                      uint32_t *__restrict__ out_base, uint32_t *__restrict__ out_shared,
                                                                                                      uint8_t *__restrict__ ok, size_t n, unsigned nb) {
    const bool shared = blockIdx.x >= nb;  // wave-uniform
    const size_t i = (size_t)(blockIdx.x - (shared ? nb : 0)) * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t k[14], u[14], r[14];
#pragma unroll
    for (int j = 0; j < 14; j++) {
        k[j] = scalar[i * 14 + j];
        u[j] = shared ? point[i * 14 + j] : 0u;
    }
    if (shared) {
        if (ok) ok[i] = (uint8_t)valid_public(u);
        scalar_mult<false>(r, k, u);
    } else if (COMB) {
        base_mult_comb(r, k);
    } else {
        scalar_mult<true>(r, k, u);
    }
    uint32_t *out = shared ? out_shared : out_base;
#pragma unroll
    for (int j = 0; j < 14; j++) out[i * 14 + j] = r[j];
}

}  // namespace x448
}  // namespace circl
