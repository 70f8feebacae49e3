// ascon_kernels.h -- batch Ascon128 / Ascon128a / Ascon80pq Seal and Open (cipher/ascon/ascon.go) over ascon_dev.h: one item per lane,
// one launch per call, no workspace, no LDS.  The mode is a template argument (block size, pB, the key's words, the key injection
// of finalize).  A wavefront runs as long as its longest item; lanes whose item is finished are predicated off.
//
// Registers: the state (10), the key (5), two row pointers and two lengths.  The kernels ask for all 8 wavefronts of a SIMD,
// __launch_bounds__(64, 8): at most 64 VGPRs, no scratch (DESIGN 4.8h has what the compiler reports).
#pragma once
#include <hip/hip_runtime.h>

#include "ascon_dev.h"

namespace circl {
namespace ascon {

struct Args {
    const uint32_t *key;       // rows of key_bytes(mode), key_stride_words apart (0: one key for the batch)
    size_t key_stride_words;
    const uint32_t *nonce;     // n rows of 16 bytes
    const uint8_t *in, *aad;   // the plaintext blob (Seal) / the ciphertext blob (Open); aad == nullptr: every aad is empty
    const uint64_t *pt_off;    // nullptr: every plaintext is empty
    const uint64_t *aad_off;
    uint8_t *out, *ok;
    size_t n;
};

// item i's plaintext is pt_off[i + 1] - pt_off[i] bytes at offset pt_off[i]; its ciphertext 16 bytes longer at pt_off[i] + 16 i
template <int MODE, bool SEAL>
CIRCL_HD void item(const Args &a, size_t i) {
    const uint32_t *key = a.key + i * a.key_stride_words, *nonce = a.nonce + 4 * i;
    const bool has_aad = a.aad && a.aad_off;
    const uint8_t *aad = has_aad ? a.aad + a.aad_off[i] : nullptr;
    const uint64_t aad_len = has_aad ? a.aad_off[i + 1] - a.aad_off[i] : 0;
    const uint64_t at = a.pt_off ? a.pt_off[i] : 0, pt_len = a.pt_off ? a.pt_off[i + 1] - at : 0;
    if (SEAL) {
        seal<MODE>(a.out + at + 16 * i, key, nonce, a.in + at, pt_len, aad, aad_len);
    } else {
        const uint32_t good = open<MODE>(a.out + at, key, nonce, a.in + at + 16 * i, pt_len, aad, aad_len);
        if (a.ok) a.ok[i] = (uint8_t)good;
    }
}

template <int MODE, bool SEAL>
static __global__ __launch_bounds__(64, 8) void kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    item<MODE, SEAL>(a, i);
}

}  // namespace ascon
}  // namespace circl
