// aesgcm_kernels.h -- batch AES-128-GCM / AES-256-GCM Seal and Open over aesgcm_dev.h: one item per lane, one launch per call, no
// workspace, no LDS.  The key size and Seal / Open are template arguments.  A wavefront runs as long as its longest item; lanes
// whose item is finished are predicated off.
//
// Registers: the compact round keys (44 / 60), the eight bit planes and the S-box circuit's live values, H, Y and E_K(J0) (12), the
// row pointers and lengths.  The kernels ask for four wavefronts a SIMD, __launch_bounds__(64) with amdgpu_waves_per_eu(4, 4): at
// most 128 VGPRs.  The compiler reports, Seal / Open: AES-128 117 / 115 VGPRs and no scratch, AES-256 128 / 127 VGPRs and 20 / 0
// bytes of scratch per lane (4 spilled VGPRs in Seal); no LDS, occupancy 4 for all four.  Asking for two wavefronts (AES-256 then
// takes 133 / 131 VGPRs, no scratch, occupancy 3) was timed against this and neither won: DESIGN 4.8i, profiles/aesgcm_bench.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "aesgcm_dev.h"

namespace circl {
namespace aesgcm {

struct Args {
    const uint32_t *key;       // rows of KEYBYTES, key_stride_words apart (0: one key for the batch)
    size_t key_stride_words;
    const uint32_t *nonce;     // rows of 12 bytes, nonce_stride_words apart (0: one base nonce for the batch; then seq != nullptr)
    size_t nonce_stride_words;
    const uint64_t *seq;       // nullptr: the row is the nonce; else the nonce is row XOR BE96(seq[i])
    const uint8_t *in, *aad;   // the plaintext blob (Seal) / the ciphertext blob (Open); aad == nullptr: every aad is empty
    const uint64_t *pt_off;    // nullptr: every plaintext is empty
    const uint64_t *aad_off;
    uint8_t *out, *ok;
    size_t n;
};

// item i's plaintext is pt_off[i + 1] - pt_off[i] bytes at offset pt_off[i]; its ciphertext 16 bytes longer at pt_off[i] + 16 i
template <int KEYBYTES, bool SEAL>
CIRCL_HD void item(const Args &a, size_t i) {
    const uint32_t *key = a.key + i * a.key_stride_words, *row = a.nonce + i * a.nonce_stride_words;
    uint32_t nonce[3] = {row[0], row[1], row[2]};
    if (a.seq) chapoly::seq_nonce(nonce, row, a.seq[i]);
    const bool has_aad = a.aad && a.aad_off;
    const uint8_t *aad = has_aad ? a.aad + a.aad_off[i] : nullptr;
    const uint64_t aad_len = has_aad ? a.aad_off[i + 1] - a.aad_off[i] : 0;
    const uint64_t at = a.pt_off ? a.pt_off[i] : 0, pt_len = a.pt_off ? a.pt_off[i + 1] - at : 0;
    if (SEAL) {
        seal<KEYBYTES>(a.out + at + 16 * i, key, nonce, a.in + at, pt_len, aad, aad_len, 0xffffffffu);
    } else {
        const uint32_t good = open<KEYBYTES>(a.out + at, key, nonce, a.in + at + 16 * i, pt_len, aad, aad_len, 1u);
        if (a.ok) a.ok[i] = (uint8_t)good;
    }
}

template <int KEYBYTES, bool SEAL>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    item<KEYBYTES, SEAL>(a, i);
}

}  // namespace aesgcm
}  // namespace circl
