// tests/hostsim/dleq_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/dleq_group_kernels.h on the CPU (their host instantiation for ristretto255): the element function of the composite
// kernel, both tails of the finish kernel and the POPRF item functions, so that the CPU-only test tier can check the very source the
// kernels are built from against the checker tests/dleq.py.  The partial sums are added one after the other here; the shuffle tree of
// the composite kernel is device code and is covered by tests/test_gpu_dleq.py.  Nothing here is linked into libcirclhip.so.
//
// With -DDLEQ_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: blobs and element arrays are heap blocks of exactly their
// size, requests of 1, 2 and 5 elements are proven and verified, and the POPRF items must agree with each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

// (see oprf_hostsim.hip: host-only, so plain inline instead of the device's forced inlining)
#define CIRCL_HD __host__ __device__ inline

#include "dleq_group_kernels.h"

using namespace circl;
using ed25519::Ge;
using oprf::R255;
using O = gdleq::Ops<R255>;

extern "C" {

uint64_t hs_dleq_request_of(const gdleq::Args *a, uint64_t e) { return gdleq::request_of<R255>(*a, e); }

// the element function: m and z as 40 words each; returns its verdict
int hs_dleq_element(int verify, const gdleq::Args *a, uint64_t g, uint64_t e, uint32_t *m, uint32_t *z) {
    Ge pm, pz;
    const uint32_t good = verify ? gdleq::element<R255, true>(pm, pz, *a, g, e) : gdleq::element<R255, false>(pm, pz, *a, g, e);
    O::store(m, pm);
    O::store(z, pz);
    return (int)good;
}

// One whole call the way the two kernels run it, one lane after the other: every element through element<>, the request's flag, the
// sums in element order, then the tail.  a->bad must hold n_req words; a->partial is not used.
void hs_dleq_call(int verify, const gdleq::Args *a) {
    const uint64_t e0 = gdleq::elem_off<R255>(*a, 0);
    for (size_t g = 0; g < a->n_req; g++) a->bad[g] = 0;
    for (size_t g = 0; g < a->n_req; g++) {
        const uint64_t first = gdleq::elem_off<R255>(*a, g), cnt = gdleq::elem_off<R255>(*a, g + 1) - first;
        Ge M = ed25519::ge_identity(), Z = ed25519::ge_identity();
        for (uint64_t e = first; e < first + cnt && e - e0 < a->n_elems; e++) {
            if (gdleq::request_of<R255>(*a, e) != g) a->bad[g] = 1u;   // (the search must find the request that owns e)
            Ge pm, pz;
            const uint32_t good = verify ? gdleq::element<R255, true>(pm, pz, *a, g, e) : gdleq::element<R255, false>(pm, pz, *a, g, e);
            if (!good) a->bad[g] = 1u;
            M = r255::r255_add(M, pm);
            if (verify) Z = r255::r255_add(Z, pz);
        }
        const uint32_t good = (cnt >= 1 && cnt <= gdleq::kMaxBatch && !a->bad[g]) ? 1u : 0u;
        if (!good) M = Z = ed25519::ge_identity();
        if (verify) gdleq::verify_tail<R255>(*a, g, M, Z, good);
        else gdleq::prove_tail<R255>(*a, g, M, good);
    }
}

void hs_poprf_item(int op, const gdleq::ItemArgs *a, uint64_t i) {
    switch (op) {
        case gdleq::kTweakServer: gdleq::PoprfItem<R255, gdleq::kTweakServer>::run(*a, i); break;
        case gdleq::kTweakClient: gdleq::PoprfItem<R255, gdleq::kTweakClient>::run(*a, i); break;
        case gdleq::kPoprfFinalize: gdleq::PoprfItem<R255, gdleq::kPoprfFinalize>::run(*a, i); break;
        case gdleq::kPoprfFullEvaluate: gdleq::PoprfItem<R255, gdleq::kPoprfFullEvaluate>::run(*a, i); break;
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

uint8_t *bytes(uint32_t *w) { return reinterpret_cast<uint8_t *>(w); }

int fail(const char *what) {
    printf("FAIL %s\n", what);
    return 1;
}

void set_tag(gdleq::Args &a, int mode) {
    const char *s = "HashToScalar-OPRFV1-";
    size_t at = 0;
    for (; *s; s++) a.tag[at++] = (uint8_t)*s;
    a.tag[at++] = (uint8_t)mode;
    for (s = R255::ctx_tail(); *s; s++) a.tag[at++] = (uint8_t)*s;
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
    gdleq::Args a = {};
    a.off = offs.data(); a.off_div = 1;
    a.B = bytes(B.w); a.kB = bytes(kB.w); a.k = k.w; a.k_stride = 8; a.kA = bytes(kA.w); a.kA_stride = 32; a.r = r.w; a.proofs = proofs.w; a.ok = ok.data();
    a.bad = bad.w; a.n_req = n_req; a.n_elems = n; a.flags = gdleq::kNoIdentity;
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
    gdleq::ItemArgs a = {};
    a.info = info.p; a.info_off = info_off.data(); a.scalars = sk.w; a.scalar_stride = 0; a.out = bytes(t.w); a.out2 = bytes(tinv.w); a.out3 = bytes(tg.w);
    a.ok = ok.data(); a.n = n;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(gdleq::kTweakServer, &a, i); if (!ok[i]) return fail("tweak (server) refused an item"); }
    a.scalars = nullptr; a.elems = bytes(pk.w); a.elem_stride = 0; a.out = bytes(tweaked.w); a.out2 = a.out3 = nullptr;
    for (size_t i = 0; i < n; i++) { hs_poprf_item(gdleq::kTweakClient, &a, i); if (!ok[i]) return fail("tweak (client) refused an item"); }
    if (memcmp(tg.w, tweaked.w, 32 * n)) return fail("t G != m G + pkS");
    // blind, evaluate with t^-1 (base-mode items of oprf_group_kernels.h), finalize with the info; and the same in one step
    for (size_t i = 0; i < n; i++) small_scalar(blinds.w + 8 * i, 500 + (uint32_t)i);
    oprf::Args o = {};
    o.blob = in.p; o.off = in_off.data(); o.scalars = blinds.w; o.scalar_stride = 8; o.out = bytes(blinded.w); o.ok = ok.data(); o.n = n;
    o.dst_len = gdleq::mode2_tag<R255>(o.dst, true);
    for (size_t i = 0; i < n; i++) { oprf::Item<oprf::R255, oprf::kBlind, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("blind refused an item"); }
    o.blob = nullptr; o.off = nullptr; o.scalars = tinv.w; o.elems = bytes(blinded.w); o.out = bytes(evaluated.w);
    for (size_t i = 0; i < n; i++) { oprf::Item<oprf::R255, oprf::kEvaluate, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("evaluate refused an item"); }
    a.input = in.p; a.input_off = in_off.data(); a.scalars = blinds.w; a.scalar_stride = 8; a.elems = bytes(evaluated.w); a.elem_stride = 32; a.out = bytes(out.w);
    for (size_t i = 0; i < n; i++) { hs_poprf_item(gdleq::kPoprfFinalize, &a, i); if (!ok[i]) return fail("poprf_finalize refused an item"); }
    a.scalars = sk.w; a.scalar_stride = 0; a.elems = nullptr; a.out = bytes(full.w);
    for (size_t i = 0; i < n; i++) { hs_poprf_item(gdleq::kPoprfFullEvaluate, &a, i); if (!ok[i]) return fail("poprf_full_evaluate refused an item"); }
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
