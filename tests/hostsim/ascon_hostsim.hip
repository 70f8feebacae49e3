// tests/hostsim/ascon_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ item functions of
// circl_amd/csrc/ascon_kernels.h on the CPU (their host instantiation), so that the CPU-only test tier can check the very source the
// kernels are built from against the checker tests/ascon.py and the reference's vectors.  Nothing here is linked into libcirclhip.so.
//
// With -DASCON_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: blobs are heap blocks of exactly their size, every mode
// seals and opens a ragged batch at odd offsets, and a tampered item must fail alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "ascon_kernels.h"

using namespace circl;

extern "C" {

// one whole call the way the kernel runs it, one lane after the other; returns 0, or -1 for an unknown mode
int hs_ascon_call(int mode, int seal, const ascon::Args *a) {
    for (size_t i = 0; i < a->n; i++) {
        switch (mode) {
            case ascon::ASCON128: seal ? ascon::item<ascon::ASCON128, true>(*a, i) : ascon::item<ascon::ASCON128, false>(*a, i); break;
            case ascon::ASCON128A: seal ? ascon::item<ascon::ASCON128A, true>(*a, i) : ascon::item<ascon::ASCON128A, false>(*a, i); break;
            case ascon::ASCON80PQ: seal ? ascon::item<ascon::ASCON80PQ, true>(*a, i) : ascon::item<ascon::ASCON80PQ, false>(*a, i); break;
            default: return -1;
        }
    }
    return 0;
}

// the permutation alone: s = five 64-bit words
void hs_ascon_perm(int rounds, uint64_t *s) {
    ascon::State st;
    for (int j = 0; j < 5; j++) {
        st.lo[j] = (uint32_t)s[j];
        st.hi[j] = (uint32_t)(s[j] >> 32);
    }
    if (rounds == 12) ascon::perm<12>(st);
    else if (rounds == 8) ascon::perm<8>(st);
    else ascon::perm<6>(st);
    for (int j = 0; j < 5; j++) s[j] = (uint64_t)st.hi[j] << 32 | st.lo[j];
}

}  // extern "C"

#ifdef ASCON_HOSTSIM_MAIN
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

int fail(const char *what, int mode) {
    printf("FAIL mode %d: %s\n", mode, what);
    return 1;
}

int run_mode(int mode, size_t lead) {
    const size_t n = 11, ks = (size_t)ascon::key_bytes(mode);
    const size_t pt_len[n] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 70}, aad_len[n] = {0, 1, 8, 13, 16, 17, 40, 0, 7, 15, 32};
    std::vector<uint64_t> pt_off(n + 1, lead), aad_off(n + 1, 3);
    for (size_t i = 0; i < n; i++) {
        pt_off[i + 1] = pt_off[i] + pt_len[i];
        aad_off[i + 1] = aad_off[i] + aad_len[i];
    }
    Bytes keys(n * ks, 11), nonces(n * 16, 12), pt(pt_off[n], 13), aad(aad_off[n], 14), ct(pt_off[n] + 16 * n), back(pt_off[n] ? pt_off[n] : 0);
    std::vector<uint8_t> ok(n, 7);
    ascon::Args a = {};
    a.key = reinterpret_cast<const uint32_t *>(keys.p); a.key_stride_words = ks / 4; a.nonce = reinterpret_cast<const uint32_t *>(nonces.p);
    a.in = pt.p; a.aad = aad.p; a.pt_off = pt_off.data(); a.aad_off = aad_off.data(); a.out = ct.p; a.n = n;
    if (hs_ascon_call(mode, 1, &a)) return fail("seal", mode);
    a.in = ct.p; a.out = back.p; a.ok = ok.data();
    if (hs_ascon_call(mode, 0, &a)) return fail("open", mode);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != 1) return fail("open refused a good item", mode);
    if (memcmp(back.p + lead, pt.p + lead, pt_off[n] - lead)) return fail("open(seal(pt)) != pt", mode);
    // one flipped tag bit in item 5: that item alone fails and its row is cleared
    ct.p[pt_off[6] + 16 * 5 + 3] ^= 0x10;
    if (hs_ascon_call(mode, 0, &a)) return fail("open", mode);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != (i == 5 ? 0 : 1)) return fail("the verdicts after tampering", mode);
    for (size_t o = pt_off[5]; o < pt_off[6]; o++)
        if (back.p[o]) return fail("a failed item's plaintext row is not zero", mode);
    if (memcmp(back.p + pt_off[6], pt.p + pt_off[6], pt_off[n] - pt_off[6])) return fail("tampering disturbed a neighbour", mode);
    // empty plaintexts without a blob, one key for the batch: n tags, and they open
    Bytes tags(16 * n);
    ascon::Args e = {};
    e.key = a.key; e.key_stride_words = 0; e.nonce = a.nonce; e.aad = aad.p; e.aad_off = aad_off.data(); e.out = tags.p; e.n = n;
    if (hs_ascon_call(mode, 1, &e)) return fail("seal (empty)", mode);
    e.in = tags.p; e.out = nullptr; e.ok = ok.data();
    if (hs_ascon_call(mode, 0, &e)) return fail("open (empty)", mode);
    for (size_t i = 0; i < n; i++)
        if (ok[i] != 1) return fail("open refused an empty item", mode);
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    for (int mode : {ascon::ASCON128, ascon::ASCON128A, ascon::ASCON80PQ})
        for (size_t lead : {size_t(0), size_t(5)}) bad |= run_mode(mode, lead);
    puts(bad ? "ascon_hostsim: FAILED" : "ascon_hostsim: ok");
    return bad;
}
#endif
