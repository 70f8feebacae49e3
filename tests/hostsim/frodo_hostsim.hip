// tests/hostsim/frodo_hostsim.hip -- TEST INFRASTRUCTURE: runs the __host__ __device__ functions of circl_amd/csrc/frodo_dev.h on the
// CPU (their host instantiation), so that the CPU-only test tier can check the very source the FrodoKEM kernels are built from
// against tests/frodo.py.  The per-item stages (keygen_pre / keygen_post, encaps_pre, decaps_pre, shared_secret) are the device's own;
// the matrix kernels, which live on LDS and many lanes, are stood in for by plain loops over rows squeezed with a_row_init and
// keccak_f1600 and packed with pack8, in the workspace layout the kernels use.  Nothing here is linked into libcirclhip.so.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "frodo_dev.h"

using namespace circl;
using namespace circl::frodo;

namespace {
void a_row(uint16_t *out, const uint32_t seed_a[4], uint32_t i) {
    KeccakState st;
    a_row_init(st, i, seed_a);
    for (int blk = 0; blk < kRowBlocks; blk++) {
        keccak_f1600(st);
        for (int d = 0; d < kBlockPairs; d++) {
            const int jp = blk * kBlockPairs + d;
            if (jp >= kRowPairs) break;
            const uint32_t w = (d & 1) ? st.hi[d >> 1] : st.lo[d >> 1];
            out[2 * jp] = (uint16_t)w;
            out[2 * jp + 1] = (uint16_t)(w >> 16);
        }
    }
}
void pack_words(uint8_t *out, const uint16_t *v, int n) {
    for (int g = 0; g < n / 8; g++) {
        uint32_t w[8], d[4];
        for (int m = 0; m < 8; m++) w[m] = v[8 * g + m];
        pack8(d, w);
        st15(out + 15 * g, d);
    }
}
// what frodo_encaps_matrix_kernel computes: B' || C packed, from the noise row, the pk and mu
void encrypt_matrix(uint8_t *out, const uint8_t *pk, const uint8_t *mu, const uint32_t *noise) {
    const uint16_t *nz = reinterpret_cast<const uint16_t *>(noise);
    const uint16_t *sp = nz, *ep = nz + kNbar * kN, *epp = nz + 2 * kNbar * kN;
    uint32_t seed_a[4], m4[4];
    for (int j = 0; j < 4; j++) { seed_a[j] = ld32u(pk + 4 * j); m4[j] = ld32u(mu + 4 * j); }
    std::vector<uint16_t> bp(ep, ep + kNbar * kN), row(kN);
    uint16_t v[kNbar * kNbar];
    for (int e = 0; e < kNbar * kNbar; e++) v[e] = epp[e];
    for (int j = 0; j < kN; j++) {
        a_row(row.data(), seed_a, (uint32_t)j);
        uint32_t d[4], b[8];
        ld15(d, pk + kSeedA + 15 * j);
        unpack8(b, d);
        for (int k = 0; k < kNbar; k++) {
            const uint16_t s = sp[k * kN + j];
            for (int i = 0; i < kN; i++) bp[k * kN + i] = (uint16_t)(bp[k * kN + i] + s * row[i]);
            for (int i = 0; i < kNbar; i++) v[k * kNbar + i] = (uint16_t)(v[k * kNbar + i] + s * b[i]);
        }
    }
    pack_words(out, bp.data(), kNbar * kN);
    uint16_t c[kNbar * kNbar];
    for (int e = 0; e < kNbar * kNbar; e++) c[e] = (uint16_t)((v[e] & kQMask) + encode_entry(m4, e));
    pack_words(out + kBPacked, c, kNbar * kNbar);
}
}  // namespace

extern "C" {

uint32_t hs_frodo_sample_pair(uint32_t w) { return sample_pair(w); }
void hs_frodo_pack8(uint8_t *out15, const uint32_t *v) {
    uint32_t d[4];
    pack8(d, v);
    st15(out15, d);
}
void hs_frodo_unpack8(uint32_t *v, const uint8_t *in15) {
    uint32_t d[4];
    ld15(d, in15);
    unpack8(v, d);
}
uint32_t hs_frodo_encode_entry(const uint32_t *mu, int e) { return encode_entry(mu, e); }
uint32_t hs_frodo_decode_entry(uint32_t w) { return decode_entry(w); }
uint32_t hs_frodo_ld32u(const uint8_t *p) { return ld32u(p); }
// nwords dwords of a row of nbytes through RowReader
void hs_frodo_row_reader(uint32_t *out, const uint8_t *p, uint32_t nbytes) {
    RowReader rd(p, nbytes);
    for (uint32_t i = 0; i < nbytes / 4; i++) out[i] = rd.word();
}
void hs_frodo_hash_row16(uint32_t *out, const uint8_t *row, uint32_t nbytes) { hash_row16(out, row, nbytes); }
void hs_frodo_a_row(uint16_t *out, const uint8_t *seed_a16, uint32_t i) {
    uint32_t sa[4];
    for (int j = 0; j < 4; j++) sa[j] = ld32u(seed_a16 + 4 * j);
    a_row(out, sa, i);
}

void hs_frodo_keygen(const uint8_t *seed48, uint8_t *pk, uint8_t *sk) {
    std::vector<uint32_t> noise(kNoiseRow / 4);
    keygen_pre(seed48, pk, sk, noise.data());
    // frodo_keygen_matrix_kernel
    const uint16_t *st = reinterpret_cast<const uint16_t *>(noise.data()), *e = st + kNbar * kN;
    memcpy(sk + kSkS, st, 2 * kNbar * kN);
    uint32_t seed_a[4];
    for (int j = 0; j < 4; j++) seed_a[j] = ld32u(pk + 4 * j);
    std::vector<uint16_t> row(kN);
    for (int i = 0; i < kN; i++) {
        a_row(row.data(), seed_a, (uint32_t)i);
        uint32_t b[8], d[4];
        for (int k = 0; k < kNbar; k++) {
            uint16_t sum = e[i * kNbar + k];
            for (int j = 0; j < kN; j++) sum = (uint16_t)(sum + row[j] * st[k * kN + j]);
            b[k] = sum;
        }
        pack8(d, b);
        st15(pk + kSeedA + 15 * i, d);
        st15(sk + kSs + kSeedA + 15 * i, d);
    }
    keygen_post(pk, sk);
}
void hs_frodo_encaps(const uint8_t *pk, const uint8_t *mu16, uint8_t *ct, uint8_t *ss) {
    std::vector<uint32_t> noise(kNoiseRow / 4);
    uint32_t k[4];
    encaps_pre(pk, mu16, noise.data(), k);
    encrypt_matrix(ct, pk, mu16, noise.data());
    shared_secret<false>(ss, ct, k, nullptr, nullptr);
}
void hs_frodo_decaps(const uint8_t *sk, const uint8_t *ct, uint8_t *ss) {
    std::vector<uint32_t> noise(kNoiseRow / 4), ct2(kCt / 4);
    uint32_t k[4], mu[4];
    decaps_pre(sk, ct, noise.data(), k, mu);
    encrypt_matrix(reinterpret_cast<uint8_t *>(ct2.data()), sk + kSs, reinterpret_cast<const uint8_t *>(mu), noise.data());
    shared_secret<true>(ss, ct, k, ct2.data(), sk);
}

}  // extern "C"
