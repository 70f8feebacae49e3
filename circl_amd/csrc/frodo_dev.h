// frodo_dev.h -- FrodoKEM-640-SHAKE (kem/frodo/frodo640shake): the lane-local pieces.  Everything here is __host__ __device__, so
// tests/hostsim/frodo_hostsim.hip runs the very same source on the CPU.
//
// The reference's behaviour that is its own and is reproduced here word for word:
//   * A's words are the raw 16-bit SHAKE128 output (matrix_shake.go), never reduced;
//   * products and sums are taken mod 2^16; the 15-bit mask is applied only by pack, add / sub, mulAddSBPlusE, mulBS and the explicit
//     mask on BB' (util.go, frodo.go) -- since pack masks, comparing packed bytes is comparing the masked words;
//   * a private key's S words are arbitrary uint16 and multiply as such; the hpk stored in the key is used as it is;
//   * the sampler is the 12-comparison sum of noise.go with the sign from bit 0; decode adds 2^12 and takes bits 13-14.
//
// Alignment promise of the row readers: NONE is needed.  ld32u / RowReader read the aligned dwords that hold a byte of the row (and
// only those), so item rows of 9616, 9720 or 19888 bytes may start at any byte; outputs are written byte by byte.
// Secrets never steer a branch or an address: the sampler, the compare and the select are arithmetic.
#pragma once
#include "keccak_dev.h"

namespace circl {
namespace frodo {

// ---- the parameter set, in one place (FrodoKEM-976 / -1344 would be other values of these) -------------------------------------
constexpr int kN = 640, kNbar = 8, kLogQ = 15, kB = 2;
constexpr uint32_t kQMask = (1u << kLogQ) - 1;
constexpr int kSeedA = 16, kHpk = 16, kMu = 16, kSs = 16;
constexpr int kBPacked = kLogQ * kN * kNbar / 8;                     // 9600: pack15 of an N x nbar (or nbar x N) matrix
constexpr int kCPacked = kLogQ * kNbar * kNbar / 8;                  // 120
constexpr int kPk = kSeedA + kBPacked;                               // 9616
constexpr int kSk = kSs + kPk + 2 * kN * kNbar + kHpk;               // 19888
constexpr int kCt = kBPacked + kCPacked;                             // 9720
constexpr int kSkS = kSs + kPk;                                      // 9632: where transpose(S) starts in a private key
constexpr int kSkHpk = kSk - kHpk;
constexpr int kKeygenNoiseWords = 2 * kN * kNbar;                    // S^T, E
constexpr int kEncNoiseWords = 2 * kN * kNbar + kNbar * kNbar;       // S', E', E''
constexpr int kNoiseRow = 2 * kEncNoiseWords;                        // 20608 bytes of workspace per item (16-byte multiple)
constexpr int kRowBlocks = (2 * kN + 167) / 168;                     // 8 SHAKE128 blocks per row of A
constexpr int kBlockPairs = 42;                                      // column pairs (dwords) per block
constexpr int kRowPairs = kN / 2;                                    // 320
static_assert(kNoiseRow % 16 == 0 && kN % 64 == 0 && kN % 8 == 0, "layout");

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
CIRCL_HD u16x2 as_pair(uint32_t w) { u16x2 r; r.x = (uint16_t)w; r.y = (uint16_t)(w >> 16); return r; }
CIRCL_HD uint32_t as_word(u16x2 p) { return (uint32_t)p.x | ((uint32_t)p.y << 16); }

// ---- noise.go sample on the two 16-bit words of a dword ------------------------------------------------------------------------
CIRCL_HD uint32_t sample_pair(uint32_t w) {
    constexpr uint16_t cdf[12] = {4643, 13363, 20579, 25843, 29227, 31145, 32103, 32525, 32689, 32745, 32762, 32766};
    const u16x2 x = as_pair(w);
    const u16x2 one = {1, 1}, sh1 = {1, 1}, sh15 = {15, 15}, zero = {0, 0};
    const u16x2 sign = x & one, u = x >> sh1;
    u16x2 g = zero;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const u16x2 c = {cdf[j], cdf[j]};
        g += (c - u) >> sh15;
    }
    return as_word(((zero - sign) ^ g) + sign);
}

// ---- util.go pack / unpack: eight 15-bit words <-> 15 bytes, most significant bit first ------------------------------------------
// The 15 bytes travel as four little-endian dwords (byte 15, the top byte of d[3], is zero / ignored).
CIRCL_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
CIRCL_HD void pack8(uint32_t d[4], const uint32_t v[8]) {
    uint64_t hi = 0, lo = 0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const uint64_t x = v[m] & kQMask;
        const int p = 15 * m;
        if (p + 15 <= 64) hi |= x << (64 - p - 15);
        else if (p >= 64) lo |= x << (128 - p - 15);
        else { hi |= x >> (p + 15 - 64); lo |= x << (128 - p - 15); }
    }
    d[0] = bswap32((uint32_t)(hi >> 32)); d[1] = bswap32((uint32_t)hi);
    d[2] = bswap32((uint32_t)(lo >> 32)); d[3] = bswap32((uint32_t)lo) & 0x00ffffffu;
}
CIRCL_HD void unpack8(uint32_t v[8], const uint32_t d[4]) {
    const uint64_t hi = ((uint64_t)bswap32(d[0]) << 32) | bswap32(d[1]);
    const uint64_t lo = ((uint64_t)bswap32(d[2]) << 32) | bswap32(d[3] & 0x00ffffffu);
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int p = 15 * m;
        uint64_t x;
        if (p + 15 <= 64) x = hi >> (64 - p - 15);
        else if (p >= 64) x = lo >> (128 - p - 15);
        else x = (hi << (p + 15 - 64)) | (lo >> (128 - p - 15));
        v[m] = (uint32_t)x & kQMask;
    }
}

// ---- util.go encodeMessage / decodeMessage, one entry --------------------------------------------------------------------------
// entry e = 8 k + i of the 8 x 8 matrix carries bits 2 i, 2 i + 1 of the k-th 16-bit word of mu
CIRCL_HD uint32_t encode_entry(const uint32_t mu[4], int e) {
    const uint32_t word16 = (mu[e >> 4] >> (16 * ((e >> 3) & 1))) & 0xffffu;
    return ((word16 >> (2 * (e & 7))) & 3u) << (kLogQ - kB);
}
CIRCL_HD uint32_t decode_entry(uint32_t w) { return ((((w & kQMask) + (1u << (kLogQ - kB - 1))) & 0xffffu) >> (kLogQ - kB)) & 3u; }

// ---- bytes at any alignment ----------------------------------------------------------------------------------------------------
// the little-endian dword at p: the one or two aligned dwords that hold its bytes
CIRCL_HD uint32_t ld32u(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), base = a & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)(a & 3) * 8;
    const uint32_t w0 = *reinterpret_cast<const uint32_t *>(base);
    const uint32_t w1 = sh ? *reinterpret_cast<const uint32_t *>(base + 4) : 0u;
    return alignbit(w1, w0, sh);
}
CIRCL_HD void ld15(uint32_t d[4], const uint8_t *p) {  // fifteen bytes, none behind them
    d[0] = ld32u(p); d[1] = ld32u(p + 4); d[2] = ld32u(p + 8);
    d[3] = (uint32_t)p[12] | ((uint32_t)p[13] << 8) | ((uint32_t)p[14] << 16);
}
CIRCL_HD void st32u(uint8_t *p, uint32_t w) {
    p[0] = (uint8_t)w; p[1] = (uint8_t)(w >> 8); p[2] = (uint8_t)(w >> 16); p[3] = (uint8_t)(w >> 24);
}
CIRCL_HD void st15(uint8_t *p, const uint32_t d[4]) {
#pragma unroll
    for (int b = 0; b < 15; b++) p[b] = (uint8_t)(d[b >> 2] >> (8 * (b & 3)));
}
// consecutive dwords of a row whose length is a multiple of four, from any starting byte
struct RowReader {
    const uint32_t *next;  // the aligned dword behind `prev`
    uintptr_t end;         // first byte behind the row
    uint32_t prev, sh;
    CIRCL_HD RowReader(const uint8_t *p, uint32_t nbytes) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        next = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        end = a + nbytes;
        sh = (uint32_t)(a & 3) * 8;
        prev = *next++;
    }
    CIRCL_HD uint32_t word() {
        const uint32_t nx = reinterpret_cast<uintptr_t>(next) < end ? *next : 0u;  // (a dword is read only if it holds a byte of the row)
        next++;
        const uint32_t w = alignbit(nx, prev, sh);
        prev = nx;
        return w;
    }
};

// ---- SHAKE128 ------------------------------------------------------------------------------------------------------------------
CIRCL_HD void xor_dword(KeccakState &st, int d, uint32_t w) {  // d is a compile-time constant at every call site
    if (d & 1) st.hi[d >> 1] ^= w;
    else st.lo[d >> 1] ^= w;
}
// SHAKE128 of a message of `ndw` dwords given by src(0), src(1), ... (called in that order, once each); returns the state after the
// last permutation, whose first words are the output.
template <class Src> CIRCL_HD void shake128_dwords(KeccakState &st, int ndw, Src &&src) {
    keccak_zero(st);
    const int nblocks = ndw / 42 + 1;
#pragma unroll 1
    for (int blk = 0; blk < nblocks; blk++) {
        const int base = blk * 42;
        if (base + 42 <= ndw) {
            detail::static_for<0, 42>([&](auto ic) { xor_dword(st, decltype(ic)::v, src(base + decltype(ic)::v)); });
        } else {
            detail::static_for<0, 42>([&](auto ic) {
                constexpr int d = decltype(ic)::v;
                if (base + d < ndw) xor_dword(st, d, src(base + d));
                else if (base + d == ndw) xor_dword(st, d, kDsShake);
            });
            st.hi[20] ^= 0x80000000u;
        }
        keccak_f1600(st);
    }
}
CIRCL_HD void out16(uint32_t o[4], const KeccakState &st) { o[0] = st.lo[0]; o[1] = st.hi[0]; o[2] = st.lo[1]; o[3] = st.hi[1]; }
CIRCL_HD uint32_t pick4(const uint32_t v[4], int i) {  // by compares, never by an address (v may be secret)
    uint32_t r = v[0];
    r = i == 1 ? v[1] : r; r = i == 2 ? v[2] : r; r = i == 3 ? v[3] : r;
    return r;
}
// SHAKE128(row)[:16] of a row of nbytes (a multiple of four): H(pk)
CIRCL_HD void hash_row16(uint32_t out[4], const uint8_t *row, uint32_t nbytes) {
    KeccakState st;
    RowReader rd(row, nbytes);
    shake128_dwords(st, (int)(nbytes / 4), [&](int) { return rd.word(); });
    out16(out, st);
}
// seedSE || k = SHAKE128(hpk || mu)[:32]
CIRCL_HD void g2(uint32_t seed_se[4], uint32_t k[4], const uint32_t hpk[4], const uint32_t mu[4]) {
    KeccakState st;
    keccak_zero(st);
    st.lo[0] = hpk[0]; st.hi[0] = hpk[1]; st.lo[1] = hpk[2]; st.hi[1] = hpk[3];
    st.lo[2] = mu[0]; st.hi[2] = mu[1]; st.lo[3] = mu[2]; st.hi[3] = mu[3];
    st.lo[4] = kDsShake; st.hi[20] = 0x80000000u;
    keccak_f1600(st);
    out16(seed_se, st);
    k[0] = st.lo[2]; k[1] = st.hi[2]; k[2] = st.lo[3]; k[3] = st.hi[3];
}
// The noise stream: SHAKE128(prefix || seedSE), its first `ndwords` dwords sampled pairwise into out[0 .. ndwords) (4-byte aligned).
CIRCL_HD void noise_stream(uint32_t *out, uint32_t prefix, const uint32_t seed[4], int ndwords) {
    KeccakState st;
    keccak_zero(st);
    st.lo[0] = prefix | (seed[0] << 8);
    st.hi[0] = (seed[0] >> 24) | (seed[1] << 8);
    st.lo[1] = (seed[1] >> 24) | (seed[2] << 8);
    st.hi[1] = (seed[2] >> 24) | (seed[3] << 8);
    st.lo[2] = (seed[3] >> 24) | (kDsShake << 8);
    st.hi[20] = 0x80000000u;
#pragma unroll 1
    for (int base = 0; base < ndwords; base += 42) {
        keccak_f1600(st);
        detail::static_for<0, 21>([&](auto ic) {
            constexpr int w = decltype(ic)::v;
            if (base + 2 * w < ndwords) out[base + 2 * w] = sample_pair(st.lo[w]);
            if (base + 2 * w + 1 < ndwords) out[base + 2 * w + 1] = sample_pair(st.hi[w]);
        });
    }
}
// The sponge of row i of A, absorbed: SHAKE128(i as two bytes || seedA); every permutation that follows yields 84 columns.
CIRCL_HD void a_row_init(KeccakState &st, uint32_t i, const uint32_t seed_a[4]) {
    keccak_zero(st);
    st.lo[0] = (i & 0xffffu) | (seed_a[0] << 16);
    st.hi[0] = (seed_a[0] >> 16) | (seed_a[1] << 16);
    st.lo[1] = (seed_a[1] >> 16) | (seed_a[2] << 16);
    st.hi[1] = (seed_a[2] >> 16) | (seed_a[3] << 16);
    st.lo[2] = (seed_a[3] >> 16) | (kDsShake << 16);
    st.hi[20] = 0x80000000u;
}

// ---- the per-item stages around the matrix kernels (one item per lane on the device) -----------------------------------------------
// KeyGen, before A: seedA = SHAKE128(z)[:16] into pk and sk, s into sk, the sampled S^T || E into the item's noise row.
CIRCL_HD void keygen_pre(const uint8_t *seed48, uint8_t *pk, uint8_t *sk, uint32_t *noise) {
    uint32_t s[4], se[4], a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { s[j] = ld32u(seed48 + 4 * j); se[j] = ld32u(seed48 + 16 + 4 * j); a[j] = ld32u(seed48 + 32 + 4 * j); }
    KeccakState st;
    keccak_zero(st);
    st.lo[0] = a[0]; st.hi[0] = a[1]; st.lo[1] = a[2]; st.hi[1] = a[3];
    st.lo[2] = kDsShake; st.hi[20] = 0x80000000u;
    keccak_f1600(st);
    out16(a, st);
#pragma unroll
    for (int j = 0; j < 4; j++) { st32u(pk + 4 * j, a[j]); st32u(sk + 4 * j, s[j]); st32u(sk + kSs + 4 * j, a[j]); }
    noise_stream(noise, 0x5fu, se, kKeygenNoiseWords / 2);
}
// KeyGen, after B: H(pk) into the key's tail
CIRCL_HD void keygen_post(const uint8_t *pk, uint8_t *sk) {
    uint32_t h[4];
    hash_row16(h, pk, kPk);
#pragma unroll
    for (int j = 0; j < 4; j++) st32u(sk + kSkHpk + 4 * j, h[j]);
}
// Encaps, before A: hpk, (seedSE, k), the sampled S' || E' || E'' into the noise row, k into the workspace
CIRCL_HD void encaps_pre(const uint8_t *pk, const uint8_t *mu16, uint32_t *noise, uint32_t *k_out) {
    uint32_t hpk[4], mu[4], se[4], k[4];
    hash_row16(hpk, pk, kPk);
#pragma unroll
    for (int j = 0; j < 4; j++) mu[j] = ld32u(mu16 + 4 * j);
    g2(se, k, hpk, mu);
#pragma unroll
    for (int j = 0; j < 4; j++) k_out[j] = k[j];
    noise_stream(noise, 0x96u, se, kEncNoiseWords / 2);
}
// Decaps, before A: W = C - B' S, mu' = decode(W), then as encaps_pre with the hpk STORED in the key
CIRCL_HD void decaps_pre(const uint8_t *sk, const uint8_t *ct, uint32_t *noise, uint32_t *k_out, uint32_t *mu_out) {
    uint32_t acc[64];
#pragma unroll
    for (int e = 0; e < 64; e++) acc[e] = 0;
#pragma unroll 1
    for (int g = 0; g < kN / 8; g++) {  // columns 8 g .. 8 g + 7 of B' and of S^T
        uint32_t s[8][4];               // S^T[j][8 g + 2 m, + 1] as stored: arbitrary uint16
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int m = 0; m < 4; m++) s[j][m] = ld32u(sk + kSkS + 2 * (j * kN + 8 * g) + 4 * m);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t d[4], b[8];
            ld15(d, ct + 15 * (i * (kN / 8) + g));
            unpack8(b, d);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t t = acc[8 * i + j];
#pragma unroll
                for (int m = 0; m < 4; m++) t += b[2 * m] * (s[j][m] & 0xffffu) + b[2 * m + 1] * (s[j][m] >> 16);
                acc[8 * i + j] = t;
            }
        }
    }
    uint32_t mu[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t d[4], c[8];
        ld15(d, ct + kBPacked + 15 * i);
        unpack8(c, d);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int e = 8 * i + j;
            const uint32_t w = (c[j] - (acc[e] & kQMask)) & kQMask;  // mulBS masks, sub masks
            mu[e >> 4] |= decode_entry(w) << (2 * (e & 15));
        }
    }
    uint32_t hpk[4], se[4], k[4];
#pragma unroll
    for (int j = 0; j < 4; j++) hpk[j] = ld32u(sk + kSkHpk + 4 * j);
    g2(se, k, hpk, mu);
#pragma unroll
    for (int j = 0; j < 4; j++) { k_out[j] = k[j]; mu_out[j] = mu[j]; }
    noise_stream(noise, 0x96u, se, kEncNoiseWords / 2);
}
// ss = SHAKE128(ct || key)[:16].  DECAPS: key = k' if the re-encryption ct2 (4-byte aligned) equals ct, else the key's s -- chosen by
// a mask, after the last ciphertext word went into the sponge.
template <bool DECAPS> CIRCL_HD void shared_secret(uint8_t *ss, const uint8_t *ct, const uint32_t k[4], const uint32_t *ct2, const uint8_t *sk) {
    uint32_t key[4], rej[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) key[j] = k[j];
    if (DECAPS) {
#pragma unroll
        for (int j = 0; j < 4; j++) rej[j] = ld32u(sk + 4 * j);
    }
    uint32_t diff = 0;
    KeccakState st;
    RowReader rd(ct, kCt);
    shake128_dwords(st, kCt / 4 + 4, [&](int idx) {
        if (idx < kCt / 4) {
            const uint32_t w = rd.word();
            if (DECAPS) diff |= w ^ ct2[idx];
            return w;
        }
        const uint32_t m = 0u - ((diff | (0u - diff)) >> 31);  // all ones when the ciphertexts differ
        return (pick4(key, idx - kCt / 4) & ~m) | (pick4(rej, idx - kCt / 4) & m);
    });
    uint32_t o[4];
    out16(o, st);
#pragma unroll
    for (int j = 0; j < 4; j++) st32u(ss + 4 * j, o[j]);
}

}  // namespace frodo
}  // namespace circl
