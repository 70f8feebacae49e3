// tests/hostsim/dleq_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/dleq_kernels.h on the CPU (their host instantiation): the element function of the composite kernel, both tails of the
// finish kernel and the POPRF item functions, so that the CPU-only test tier can check the very source the kernels are built from
// against the checker tests/dleq.py.  The partial sums are added one after the other here; the shuffle tree of the composite kernel is
// device code and is covered by tests/test_gpu_dleq.py.  Nothing here is linked into libcirclhip.so.
//
// With -DDLEQ_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: blobs and element arrays are heap blocks of exactly their
// size, requests of 1, 2 and 5 elements are proven and verified, and the POPRF items must agree with each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

// (see oprf_hostsim.hip: host-only, so plain inline instead of the device's forced inlining)
#define CIRCL_HD __host__ __device__ inline

#include "dleq_kernels.h"

using namespace circl;
using ed25519::Ge;

extern "C" {

uint64_t hs_dleq_request_of(const dleq::Args *a, uint64_t e) { return dleq::request_of(*a, e); }

// the element function: m and z as 40 words each; returns its verdict
int hs_dleq_element(int verify, const dleq::Args *a, uint64_t g, uint64_t e, uint32_t *m, uint32_t *z) {
    Ge pm, pz;
    const uint32_t good = verify ? dleq::element<true>(pm, pz, *a, g, e) : dleq::element<false>(pm, pz, *a, g, e);
    dleq::ge_store(m, pm);
    dleq::ge_store(z, pz);
    return (int)good;
}

// One whole call the way the two kernels run it, one lane after the other: every element through element<>, the request's flag, the
// sums in element order, then the tail.  a->bad must hold n_req words; a->partial is not used.
void hs_dleq_call(int verify, const dleq::Args *a) {
    const uint64_t e0 = dleq::elem_off(*a, 0);
    for (size_t g = 0; g < a->n_req; g++) a->bad[g] = 0;
    for (size_t g = 0; g < a->n_req; g++) {
        const uint64_t first = dleq::elem_off(*a, g), cnt = dleq::elem_off(*a, g + 1) - first;
        Ge M = ed25519::ge_identity(), Z = ed25519::ge_identity();
        for (uint64_t e = first; e < first + cnt && e - e0 < a->n_elems; e++) {
            if (dleq::request_of(*a, e) != g) a->bad[g] = 1u;   // (the search must find the request that owns e)
            Ge pm, pz;
            const uint32_t good = verify ? dleq::element<true>(pm, pz, *a, g, e) : dleq::element<false>(pm, pz, *a, g, e);
            if (!good) a->bad[g] = 1u;
            M = r255::r255_add(M, pm);
            if (verify) Z = r255::r255_add(Z, pz);
        }
        const uint32_t good = (cnt >= 1 && cnt <= dleq::kMaxBatch && !a->bad[g]) ? 1u : 0u;
        if (!good) M = Z = ed25519::ge_identity();
        if (verify) dleq::verify_tail(*a, g, M, Z, good);
        else dleq::prove_tail(*a, g, M, good);
    }
}

void hs_poprf_item(int op, const dleq::ItemArgs *a, uint64_t i) {
    switch (op) {
        case dleq::kTweakServer: dleq::item<dleq::kTweakServer>(*a, i); break;
        case dleq::kTweakClient: dleq::item<dleq::kTweakClient>(*a, i); break;
        case dleq::kPoprfFinalize: dleq::item<dleq::kPoprfFinalize>(*a, i); break;
        case dleq::kPoprfFullEvaluate: dleq::item<dleq::kPoprfFullEvaluate>(*a, i); break;
    }
}

}  // extern "C"

#ifdef DLEQ_HOSTSIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// exact-size heap rows of 32-bit words (so that a sanitizer sees any access past the end)
struct Rows {
    uint32_t *w;
    explicit Rows(size_t words) : w(static_cast<uint32_t *>(calloc(words ? words : 1, 4))) {}
    ~Rows() { free(w); }
    Rows(const Rows &) = delete;
};
struct Bytes {
    uint8_t *p;
    explicit Bytes(size_t n, uint32_t seed = 1) : p(static_cast<uint8_t *>(malloc(n ? n : 1))) {
        for (size_t i = 0; i < n; i++) p[i] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    }
    ~Bytes() { free(p); }
    Bytes(const Bytes &) = delete;
};

int fail(const char *what) {
    printf("FAIL %s\n", what);
    return 1;
}

void set_tag(dleq::Args &a, int mode) {
    const char *s = "HashToScalar-OPRFV1-";
    size_t at = 0;
    for (; *s; s++) a.tag[at++] = (uint8_t)*s;
    a.tag[at++] = (uint8_t)mode;
    for (s = "-ristretto255-SHA512"; *s; s++) a.tag[at++] = (uint8_t)*s;
    a.tag_len = (uint32_t)at;
}

// scalar_i = a small non-zero canonical scalar
void small_scalar(uint32_t *row, uint32_t v) {
    memset(row, 0, 32);
    row[0] = v;
    row[3] = v * 2654435761u;
}

int run_proofs() {
    const size_t n_req = 4;
    const uint64_t off[n_req + 1] = {0, 1, 3, 3, 8};   // requests of 1, 2, 0 and 5 elements
    const size_t n = 8;
    Rows k(8 * n_req), kA(8 * n_req), r(8 * n_req), B(8 * n), kB(8 * n), proofs(16 * n_req), bad(n_req);
    std::vector<uint64_t> offs(off, off + n_req + 1);
    std::vector<uint8_t> ok(n_req, 7);
    for (size_t g = 0; g < n_req; g++) {
        small_scalar(k.w + 8 * g, 3 + (uint32_t)g);
        small_scalar(r.w + 8 * g, 1000 + (uint32_t)g);
        r255::r255_encode(kA.w + 8 * g, r255::r255_base(k.w + 8 * g));
    }
    for (size_t e = 0; e < n; e++) {
        size_t g = 0;
        while (off[g + 1] <= e) g++;
        uint32_t s[8];
        small_scalar(s, 77 + (uint32_t)e);
        const Ge p = r255::r255_base(s);
        r255::r255_encode(B.w + 8 * e, p);
        r255::r255_encode(kB.w + 8 * e, r255::r255_mul(k.w + 8 * g, p));
    }
    dleq::Args a = {};
    a.off = offs.data();
    a.B = B.w; a.kB = kB.w; a.k = k.w; a.k_stride = 8; a.kA = kA.w; a.kA_stride = 8; a.r = r.w; a.proofs = proofs.w; a.ok = ok.data();
    a.bad = bad.w; a.n_req = n_req; a.n_elems = n; a.flags = dleq::kNoIdentity;
    set_tag(a, 1);
    hs_dleq_call(0, &a);
    if (ok[0] != 1 || ok[1] != 1 || ok[2] != 0 || ok[3] != 1) return fail("prove: ok");
    for (int j = 0; j < 16; j++)
        if (proofs.w[32 + j]) return fail("the empty request's proof row is not zero");
    std::vector<uint8_t> verdict(n_req, 7);
    a.ok = verdict.data();
    hs_dleq_call(1, &a);
    if (verdict[0] != 1 || verdict[1] != 1 || verdict[2] != 0 || verdict[3] != 1) return fail("verify: the verdicts");
    kB.w[8 * 5] ^= 2u;   // an element of the last request
    hs_dleq_call(1, &a);
    if (verdict[0] != 1 || verdict[1] != 1 || verdict[3] != 0) return fail("verify: a tampered element passed, or disturbed a neighbour");
    return 0;
}

int run_poprf() {
    const size_t n = 6;
    std::vector<uint64_t> in_off(n + 1, 0), info_off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        in_off[i + 1] = in_off[i] + (i == 0 ? 0 : 40 * i + 3);
        info_off[i + 1] = info_off[i] + 7 * i;
    }
    Bytes in(in_off[n], 5), info(info_off[n], 9);
    Rows sk(8), pk(8), t(8 * n), tinv(8 * n), tg(8 * n), tweaked(8 * n), blinds(8 * n), blinded(8 * n), evaluated(8 * n), out(16 * n), full(16 * n);
    std::vector<uint8_t> ok(n);
    small_scalar(sk.w, 12345);
    r255::r255_encode(pk.w, r255::r255_base(sk.w));
    dleq::ItemArgs a = {};
    a.info = info.p; a.info_off = info_off.data(); a.scalars = sk.w; a.scalar_stride = 0; a.out = t.w; a.out2 = tinv.w; a.out3 = tg.w;
    a.ok = ok.data(); a.n = n;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(dleq::kTweakServer, &a, i); if (!ok[i]) return fail("tweak (server) refused an item"); }
    a.scalars = nullptr; a.elems = pk.w; a.elem_stride = 0; a.out = tweaked.w; a.out2 = a.out3 = nullptr;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(dleq::kTweakClient, &a, i); if (!ok[i]) return fail("tweak (client) refused an item"); }
    if (memcmp(tg.w, tweaked.w, 32 * n)) return fail("t G != m G + pkS");
    // blind, evaluate with t^-1 (base-mode items of oprf_group_kernels.h), finalize with the info; and the same in one step
    for (size_t i = 0; i < n; i++) small_scalar(blinds.w + 8 * i, 500 + (uint32_t)i);
    oprf::Args o = {};
    o.blob = in.p; o.off = in_off.data(); o.scalars = blinds.w; o.scalar_stride = 8; o.out = reinterpret_cast<uint8_t *>(blinded.w); o.ok = ok.data(); o.n = n;
    o.dst_len = dleq::mode2_tag(o.dst, true);
    for (size_t i = 0; i < n; i++) { oprf::Item<oprf::R255, oprf::kBlind, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("blind refused an item"); }
    o.blob = nullptr; o.off = nullptr; o.scalars = tinv.w; o.elems = reinterpret_cast<const uint8_t *>(blinded.w); o.out = reinterpret_cast<uint8_t *>(evaluated.w);
    for (size_t i = 0; i < n; i++) { oprf::Item<oprf::R255, oprf::kEvaluate, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("evaluate refused an item"); }
    a.input = in.p; a.input_off = in_off.data(); a.scalars = blinds.w; a.scalar_stride = 8; a.elems = evaluated.w; a.elem_stride = 8; a.out = out.w;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(dleq::kPoprfFinalize, &a, i); if (!ok[i]) return fail("poprf_finalize refused an item"); }
    a.scalars = sk.w; a.scalar_stride = 0; a.elems = nullptr; a.out = full.w;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(dleq::kPoprfFullEvaluate, &a, i); if (!ok[i]) return fail("poprf_full_evaluate refused an item"); }
    if (memcmp(out.w, full.w, 64 * n)) return fail("poprf_finalize(evaluate(blind(x))) != poprf_full_evaluate(x)");
    return 0;
}

}  // namespace

int main() {
    const int bad = run_proofs() | run_poprf();
    puts(bad ? "dleq_hostsim: FAILED" : "dleq_hostsim: ok");
    return bad;
}
#endif
