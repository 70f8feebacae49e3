// frodo_kernels.h -- batch FrodoKEM-640-SHAKE.  An operation is three launches on one stream:
//
//   pre    one item per lane: the serial sponges in front of A (seedA / H(pk), G2, the 122-123 permutations of the noise stream with
//          the CDF sampler) and, for decapsulation, W = C - B' S and mu' = decode(W).  The sampled matrices go to the item's noise row
//          of the workspace.
//   matrix one WORKGROUP per item, a lane per row of A: 640 independent SHAKE128 streams on the per-lane Keccak of keccak_dev.h, each
//          squeezed block by block (168 bytes = 84 columns) and consumed at once.  A never reaches memory.
//            KeyGen  B = A S + E is row-local: eight packed accumulator pairs per lane, S^T read from LDS at a wave-uniform address.
//            Encaps  B' = S' A + E' sums over rows, i.e. over lanes: every wavefront transposes its 64-row x 84-column tile through LDS,
//                    42 lanes then own a column pair each, run down the 64 rows with S'[.][row] broadcast from LDS, and add their eight
//                    pairs into the item's 8 x 640 accumulators (32-bit LDS atomics; only the low halves count).  V = S' B + E'' rides
//                    along: 64 products per row, summed over the wavefront through the same tile.
//          The kernel packs what it computed: B into pk and sk, or B' || C into the ciphertext (decapsulation: into the workspace, as
//          the re-encryption to compare with).
//   post   one item per lane: H(pk) into the key, or ss = SHAKE128(ct || k) -- for decapsulation with the compare against the
//          re-encryption folded into the absorption and k' / s chosen by a mask.
//
// WAVES wavefronts of a matrix workgroup share the 10 row groups of 64 (WAVES divides 10).
#pragma once
#include <hip/hip_runtime.h>

#include "frodo_dev.h"

namespace circl {
namespace frodo {

constexpr int kTileStride = 43;  // dwords per tile row: odd, so that the 64 lanes of a transposing store hit 64 different banks

// ---- pre / post: one item per lane ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(64) void frodo_keygen_pre_kernel(const uint8_t *__restrict__ seed48, uint8_t *__restrict__ pk, uint8_t *__restrict__ sk,
                                                                     uint32_t *__restrict__ noise, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    keygen_pre(seed48 + i * 48, pk + i * kPk, sk + i * kSk, noise + i * (kNoiseRow / 4));
}
static __global__ __launch_bounds__(64) void frodo_keygen_post_kernel(const uint8_t *__restrict__ pk, uint8_t *__restrict__ sk, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    keygen_post(pk + i * kPk, sk + i * kSk);
}
static __global__ __launch_bounds__(64) void frodo_encaps_pre_kernel(const uint8_t *__restrict__ pk, const uint8_t *__restrict__ mu16, uint32_t *__restrict__ noise,
                                                                     uint32_t *__restrict__ k_out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    encaps_pre(pk + i * kPk, mu16 + i * kMu, noise + i * (kNoiseRow / 4), k_out + i * 4);
}
static __global__ __launch_bounds__(64) void frodo_decaps_pre_kernel(const uint8_t *__restrict__ sk, const uint8_t *__restrict__ ct, uint32_t *__restrict__ noise,
                                                                     uint32_t *__restrict__ k_out, uint32_t *__restrict__ mu_out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    decaps_pre(sk + i * kSk, ct + i * kCt, noise + i * (kNoiseRow / 4), k_out + i * 4, mu_out + i * 4);
}
template <bool DECAPS>
static __global__ __launch_bounds__(64) void frodo_ss_kernel(uint8_t *__restrict__ ss, const uint8_t *__restrict__ ct, const uint32_t *__restrict__ k,
                                                             const uint32_t *__restrict__ ct2, const uint8_t *__restrict__ sk, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t kk[4];
#pragma unroll
    for (int j = 0; j < 4; j++) kk[j] = k[i * 4 + j];
    shared_secret<DECAPS>(ss + i * kSs, ct + i * kCt, kk, DECAPS ? ct2 + i * (kCt / 4) : nullptr, DECAPS ? sk + i * kSk : nullptr);
}

// ---- KeyGen: B = A S + E ---------------------------------------------------------------------------------------------------------
// noise row: S^T as 8 x 640 words (dword k * 320 + jp holds columns 2 jp, 2 jp + 1 of row k), then E as 640 x 8 words.
template <int WAVES>
static __global__ __launch_bounds__(64 * WAVES) void frodo_keygen_matrix_kernel(uint8_t *__restrict__ pk, uint8_t *__restrict__ sk,
                                                                                const uint32_t *__restrict__ noise) {
    __shared__ uint4 s_lds[kRowPairs * 2];  // [jp][k]: the pair (S^T[k][2 jp], S^T[k][2 jp + 1]), k = 0..7 as two uint4
    const size_t item = blockIdx.x;
    const uint32_t *nz = noise + item * (kNoiseRow / 4);
    uint8_t *pk_row = pk + item * kPk, *sk_row = sk + item * kSk;
    uint32_t *s_w = reinterpret_cast<uint32_t *>(s_lds);
    for (int d = threadIdx.x; d < kNbar * kRowPairs; d += 64 * WAVES) {
        const uint32_t w = nz[d];
        s_w[(d % kRowPairs) * 8 + d / kRowPairs] = w;
        st32u(sk_row + kSkS + 4 * d, w);  // transpose(S) as 16-bit little-endian words
    }
    uint32_t seed_a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) seed_a[j] = ld32u(pk_row + 4 * j);  // written by the pre kernel
    __syncthreads();
#pragma unroll 1
    for (int row = threadIdx.x; row < kN; row += 64 * WAVES) {
        KeccakState st;
        a_row_init(st, (uint32_t)row, seed_a);
        u16x2 acc[8];
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] = as_pair(0);
#pragma unroll 1
        for (int blk = 0; blk < kRowBlocks; blk++) {
            keccak_f1600(st);
            const int base = blk * kBlockPairs;
            detail::static_for<0, kBlockPairs>([&](auto ic) {
                constexpr int d = decltype(ic)::v;
                if (base + d < kRowPairs) {  // (uniform: the last block holds 26 pairs)
                    const u16x2 a = as_pair((d & 1) ? st.hi[d >> 1] : st.lo[d >> 1]);
                    const uint4 s0 = s_lds[(base + d) * 2], s1 = s_lds[(base + d) * 2 + 1];
                    acc[0] += a * as_pair(s0.x); acc[1] += a * as_pair(s0.y); acc[2] += a * as_pair(s0.z); acc[3] += a * as_pair(s0.w);
                    acc[4] += a * as_pair(s1.x); acc[5] += a * as_pair(s1.y); acc[6] += a * as_pair(s1.z); acc[7] += a * as_pair(s1.w);
                }
            });
        }
        const uint4 e = reinterpret_cast<const uint4 *>(nz + kNbar * kRowPairs)[row];  // E[row][0..7]: eight words
        const uint32_t er[4] = {e.x, e.y, e.z, e.w};
        uint32_t b[8], d[4];
#pragma unroll
        for (int k = 0; k < 8; k++) b[k] = (uint32_t)acc[k].x + (uint32_t)acc[k].y + ((er[k >> 1] >> (16 * (k & 1))) & 0xffffu);
        pack8(d, b);
        st15(pk_row + kSeedA + 15 * row, d);
        st15(sk_row + kSs + kSeedA + 15 * row, d);
    }
}

// ---- Encaps / the re-encryption of Decaps: B' = S' A + E', C = S' B + E'' + encode(mu) ---------------------------------------------
// noise row: S' (8 x 640 words), E' (8 x 640), E'' (8 x 8).  pk: the public key the item encrypts to (pk_stride apart: rows of a pk
// batch, or the pk inside rows of an sk batch); mu: 16 bytes per item, mu_stride apart; out: B' || C packed, out_stride apart.
template <int WAVES> struct EncLds {
    uint32_t acc_b[kNbar * kN];               // B' accumulators, low halves count
    uint32_t acc_v[kNbar * kNbar];            // V accumulators
    uint32_t tile[WAVES][64 * kTileStride];   // per wavefront: 64 rows x 42 column pairs
    uint4 sp[WAVES][64];                      // per wavefront: S'[0..7][row] of its 64 rows as eight words
};
template <int WAVES>
static __global__ __launch_bounds__(64 * WAVES) void frodo_encaps_matrix_kernel(const uint8_t *__restrict__ pk, size_t pk_stride, const uint8_t *__restrict__ mu,
                                                                                size_t mu_stride, const uint32_t *__restrict__ noise,
                                                                                uint8_t *__restrict__ out, size_t out_stride) {
    __shared__ EncLds<WAVES> L;
    const size_t item = blockIdx.x;
    const uint8_t *pk_row = pk + item * pk_stride;
    const uint16_t *nz16 = reinterpret_cast<const uint16_t *>(noise + item * (kNoiseRow / 4));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *tile = L.tile[wave];
    for (int d = threadIdx.x; d < kNbar * kN; d += 64 * WAVES) L.acc_b[d] = 0;
    if (threadIdx.x < kNbar * kNbar) L.acc_v[threadIdx.x] = 0;
    uint32_t seed_a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) seed_a[j] = ld32u(pk_row + 4 * j);
    __syncthreads();
#pragma unroll 1
    for (int row = threadIdx.x; row < kN; row += 64 * WAVES) {
        // S'[k][row], k = 0..7, and the row's share of V = S' B: 64 products, summed over the wavefront through the tile
        uint32_t sv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) sv[k] = nz16[k * kN + row];
        wave_lds_order();  // the previous pass is done with sp and the tile
        L.sp[wave][lane] = make_uint4(sv[0] | (sv[1] << 16), sv[2] | (sv[3] << 16), sv[4] | (sv[5] << 16), sv[6] | (sv[7] << 16));
        {
            uint32_t d[4], b[8];
            ld15(d, pk_row + kSeedA + 15 * row);
            unpack8(b, d);
#pragma unroll
            for (int k = 0; k < 8; k++)
#pragma unroll
                for (int i = 0; i < 8; i += 2)
                    tile[lane * kTileStride + (8 * k + i) / 2] = ((sv[k] * b[i]) & 0xffffu) | ((sv[k] * b[i + 1]) << 16);
            wave_lds_order();
            if (lane < 32) {
                u16x2 t = as_pair(0);
#pragma unroll 8
                for (int r = 0; r < 64; r++) t += as_pair(tile[r * kTileStride + lane]);
                atomicAdd(&L.acc_v[2 * lane], (uint32_t)t.x);
                atomicAdd(&L.acc_v[2 * lane + 1], (uint32_t)t.y);
            }
        }
        KeccakState st;
        a_row_init(st, (uint32_t)row, seed_a);
#pragma unroll 1
        for (int blk = 0; blk < kRowBlocks; blk++) {
            keccak_f1600(st);
            const int npairs = blk < kRowBlocks - 1 ? kBlockPairs : kRowPairs - (kRowBlocks - 1) * kBlockPairs;  // 42, at last 26
            wave_lds_order();  // the tile's readers of the previous block are done
            detail::static_for<0, kBlockPairs>([&](auto ic) {
                constexpr int d = decltype(ic)::v;
                if (d < npairs) tile[lane * kTileStride + d] = (d & 1) ? st.hi[d >> 1] : st.lo[d >> 1];
            });
            wave_lds_order();
            if (lane < npairs) {  // this lane owns columns 84 blk + 2 lane, + 1
                u16x2 acc[8];
#pragma unroll
                for (int k = 0; k < 8; k++) acc[k] = as_pair(0);
#pragma unroll 4
                for (int r = 0; r < 64; r++) {
                    const u16x2 a = as_pair(tile[r * kTileStride + lane]);
                    const uint4 s = L.sp[wave][r];
                    const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const uint16_t sk_ = (uint16_t)(sw[k >> 1] >> (16 * (k & 1)));
                        const u16x2 sp2 = {sk_, sk_};
                        acc[k] += a * sp2;
                    }
                }
                const int col = 2 * (blk * kBlockPairs + lane);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    atomicAdd(&L.acc_b[k * kN + col], (uint32_t)acc[k].x);
                    atomicAdd(&L.acc_b[k * kN + col + 1], (uint32_t)acc[k].y);
                }
            }
        }
    }
    __syncthreads();
    uint8_t *out_row = out + item * out_stride;
    for (int g = threadIdx.x; g < kNbar * kN / 8; g += 64 * WAVES) {  // eight consecutive words of B' -> 15 bytes
        const uint4 e = reinterpret_cast<const uint4 *>(nz16 + kNbar * kN)[g];
        const uint32_t er[4] = {e.x, e.y, e.z, e.w};
        uint32_t v[8], d[4];
#pragma unroll
        for (int m = 0; m < 8; m++) v[m] = L.acc_b[8 * g + m] + ((er[m >> 1] >> (16 * (m & 1))) & 0xffffu);
        pack8(d, v);
        st15(out_row + 15 * g, d);
    }
    if (threadIdx.x < kNbar) {  // row k of C
        const int k = threadIdx.x;
        const uint8_t *mu_row = mu + item * mu_stride;
        uint32_t m4[4], v[8], d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) m4[j] = ld32u(mu_row + 4 * j);
        const uint4 e = reinterpret_cast<const uint4 *>(nz16 + 2 * kNbar * kN)[k];
        const uint32_t er[4] = {e.x, e.y, e.z, e.w};
        // encode_entry(m4, 8 k + i) with k a lane id: the k-th 16-bit word of mu, picked by compares
        uint32_t word16 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) word16 = k == j ? (m4[j >> 1] >> (16 * (j & 1))) & 0xffffu : word16;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t vv = (L.acc_v[8 * k + i] + ((er[i >> 1] >> (16 * (i & 1))) & 0xffffu)) & kQMask;  // mulAddSBPlusE masks
            v[i] = vv + (((word16 >> (2 * i)) & 3u) << (kLogQ - kB));                                         // add masks (pack8 does)
        }
        pack8(d, v);
        st15(out_row + kBPacked + 15 * k, d);
    }
}

}  // namespace frodo
}  // namespace circl
