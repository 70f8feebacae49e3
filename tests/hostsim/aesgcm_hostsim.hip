// tests/hostsim/aesgcm_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ item functions of
// circl_amd/csrc/aesgcm_kernels.h on the CPU (their host instantiation), so that the CPU-only test tier can check the very source the
// kernels are built from against the checker tests/aesgcm.py, libcrypto and the reference's vectors.  Nothing here is linked into
// libcirclhip.so.
//
// With -DAESGCM_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: blobs are heap blocks of exactly their size, both key
// sizes seal and open a ragged batch at odd offsets, and a tampered item must fail alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "aesgcm_kernels.h"

using namespace circl;

extern "C" {

// one whole call the way the kernel runs it, one lane after the other; returns 0, or -1 for an unknown key size
int hs_aesgcm_call(int key_bytes, int seal, const aesgcm::Args *a) {
    for (size_t i = 0; i < a->n; i++) {
        switch (key_bytes) {
            case 16: seal ? aesgcm::item<16, true>(*a, i) : aesgcm::item<16, false>(*a, i); break;
            case 32: seal ? aesgcm::item<32, true>(*a, i) : aesgcm::item<32, false>(*a, i); break;
            default: return -1;
        }
    }
    return 0;
}

// one AES block through the key schedule and a two-block pass: `in` rides in slot 0 or 1 of the pass, its complement in the other
int hs_aes_encrypt_block(int key_bytes, const uint32_t *key, const uint32_t *in, uint32_t *out, int slot) {
    uint32_t q[8];
    for (int c = 0; c < 4; c++) {
        q[2 * c + slot] = in[c];
        q[2 * c + 1 - slot] = ~in[c];
    }
    if (key_bytes == 16) {
        aesgcm::RoundKeys<16> rk;
        aesgcm::expand_key<16>(rk, key);
        aesgcm::encrypt2<16>(q, rk);
    } else if (key_bytes == 32) {
        aesgcm::RoundKeys<32> rk;
        aesgcm::expand_key<32>(rk, key);
        aesgcm::encrypt2<32>(q, rk);
    } else {
        return -1;
    }
    for (int c = 0; c < 4; c++) out[c] = q[2 * c + slot];
    return 0;
}

// out = x * h in GF(2^128); all three are blocks of 16 bytes
void hs_ghash_mul(const uint8_t *x, const uint8_t *h, uint8_t *out) {
    uint32_t y[4], hw[4];
    for (int k = 0; k < 4; k++) {
        y[k] = (uint32_t)x[4 * k] << 24 | (uint32_t)x[4 * k + 1] << 16 | (uint32_t)x[4 * k + 2] << 8 | x[4 * k + 3];
        hw[k] = (uint32_t)h[4 * k] << 24 | (uint32_t)h[4 * k + 1] << 16 | (uint32_t)h[4 * k + 2] << 8 | h[4 * k + 3];
    }
    aesgcm::ghash_mul(y, hw);
    for (int k = 0; k < 4; k++)
        for (int b = 0; b < 4; b++) out[4 * k + b] = (uint8_t)(y[k] >> (24 - 8 * b));
}

// n products in one call: x, h and out are n rows of 16 bytes
void hs_ghash_mul_many(const uint8_t *x, const uint8_t *h, uint8_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) hs_ghash_mul(x + 16 * i, h + 16 * i, out + 16 * i);
}

}  // extern "C"

#ifdef AESGCM_HOSTSIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// exact-size heap blocks (so that a sanitizer sees any access past the end)
struct Bytes {
    uint8_t *p;
    size_t n;
    explicit Bytes(size_t n_, uint32_t seed = 0) : p(static_cast<uint8_t *>(malloc(n_ ? n_ : 1))), n(n_) {
        for (size_t i = 0; i < n; i++) p[i] = seed ? (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24) : 0;
    }
    ~Bytes() { free(p); }
    Bytes(const Bytes &) = delete;
};

int fail(const char *what, int kb) {
    printf("FAIL key size %d: %s\n", kb, what);
    return 1;
}

int run_size(int kb, size_t lead, bool with_seq) {
    const size_t n = 12, ks = (size_t)kb;
    const size_t pt_len[n] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 65, 130}, aad_len[n] = {0, 1, 8, 13, 16, 17, 40, 0, 7, 15, 32, 33};
    std::vector<uint64_t> pt_off(n + 1, lead), aad_off(n + 1, 3), seq(n);
    for (size_t i = 0; i < n; i++) {
        pt_off[i + 1] = pt_off[i] + pt_len[i];
        aad_off[i + 1] = aad_off[i] + aad_len[i];
        seq[i] = i * 0x100000001ull;
    }
    Bytes keys(n * ks, 11), nonces(n * 12, 12), pt(pt_off[n], 13), aad(aad_off[n], 14), ct(pt_off[n] + 16 * n), back(pt_off[n] ? pt_off[n] : 0);
    std::vector<uint8_t> ok(n, 7);
    aesgcm::Args a = {};
    a.key = reinterpret_cast<const uint32_t *>(keys.p); a.key_stride_words = ks / 4;
    a.nonce = reinterpret_cast<const uint32_t *>(nonces.p); a.nonce_stride_words = with_seq ? 0 : 3; a.seq = with_seq ? seq.data() : nullptr;
    a.in = pt.p; a.aad = aad.p; a.pt_off = pt_off.data(); a.aad_off = aad_off.data(); a.out = ct.p; a.n = n;
    if (hs_aesgcm_call(kb, 1, &a)) return fail("seal", kb);
    a.in = ct.p; a.out = back.p; a.ok = ok.data();
    if (hs_aesgcm_call(kb, 0, &a)) return fail("open", kb);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != 1) return fail("open refused a good item", kb);
    if (memcmp(back.p + lead, pt.p + lead, pt_off[n] - lead)) return fail("open(seal(pt)) != pt", kb);
    // one flipped tag bit in item 5: that item alone fails and its row is cleared
    ct.p[pt_off[6] + 16 * 5 + 3] ^= 0x10;
    if (hs_aesgcm_call(kb, 0, &a)) return fail("open", kb);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != (i == 5 ? 0 : 1)) return fail("the verdicts after tampering", kb);
    for (size_t o = pt_off[5]; o < pt_off[6]; o++)
        if (back.p[o]) return fail("a failed item's plaintext row is not zero", kb);
    if (memcmp(back.p + pt_off[6], pt.p + pt_off[6], pt_off[n] - pt_off[6])) return fail("tampering disturbed a neighbour", kb);
    // empty plaintexts without a blob, one key for the batch: n tags, and they open
    Bytes tags(16 * n);
    aesgcm::Args e = a;
    e.key_stride_words = 0; e.in = nullptr; e.pt_off = nullptr; e.out = tags.p; e.ok = nullptr;
    if (hs_aesgcm_call(kb, 1, &e)) return fail("seal (empty)", kb);
    e.in = tags.p; e.out = nullptr; e.ok = ok.data();
    if (hs_aesgcm_call(kb, 0, &e)) return fail("open (empty)", kb);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != 1) return fail("open refused an empty item", kb);
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    for (int kb : {16, 32})
        for (size_t lead : {size_t(0), size_t(5)})
            for (bool with_seq : {false, true}) bad |= run_size(kb, lead, with_seq);
    puts(bad ? "aesgcm_hostsim: FAILED" : "aesgcm_hostsim: ok");
    return bad;
}
#endif
