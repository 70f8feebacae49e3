// tests/hostsim/dleq_nistp_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/dleq_group_kernels.h on the CPU (their host instantiation) for P-256 and P-384: the element function of the composite
// kernel, both tails of the finish kernel and the POPRF item functions, so that the CPU-only test tier can check the very source the
// kernels are built from against the checker tests/dleq_nistp.py.  The partial sums are added one after the other here; the shuffle
// tree of the composite kernel is device code and is covered by tests/test_gpu_dleq_nistp.py.  Nothing here is linked into
// libcirclhip.so.
//
// With -DDLEQ_NISTP_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: blobs and element arrays are heap blocks of exactly
// their size (element arrays of exactly n * Ne bytes at ODD addresses), requests of 1, 2, 0 and 5 pairs are proven and verified on both
// curves, and the POPRF items must agree with each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

// (see oprf_hostsim.hip: host-only, so plain inline instead of the device's forced inlining)
#define CIRCL_HD __host__ __device__ inline

#include "dleq_group_kernels.h"

using namespace circl;
namespace gq = circl::gdleq;

namespace {

template <class G>
int element(int verify, const gq::Args *a, uint64_t g, uint64_t e, uint32_t *m, uint32_t *z) {
    typename G::Point pm, pz;
    const uint32_t good = verify ? gq::element<G, true>(pm, pz, *a, g, e) : gq::element<G, false>(pm, pz, *a, g, e);
    gq::Ops<G>::store(m, pm);
    gq::Ops<G>::store(z, pz);
    return (int)good;
}

// One whole call the way the two kernels run it, one lane after the other: every element through element<>, the request's flag, the
// sums in element order, then the tail.  a->bad must hold n_req words; a->partial is not used.
template <class G>
void call(int verify, const gq::Args *a) {
    using O = gq::Ops<G>;
    const uint64_t e0 = gq::elem_off<G>(*a, 0);
    for (size_t g = 0; g < a->n_req; g++) a->bad[g] = 0;
    for (size_t g = 0; g < a->n_req; g++) {
        const uint64_t first = gq::elem_off<G>(*a, g), cnt = gq::elem_off<G>(*a, g + 1) - first;
        typename G::Point M = O::identity(), Z = O::identity();
        for (uint64_t e = first; e < first + cnt && e - e0 < a->n_elems; e++) {
            if (gq::request_of<G>(*a, e) != g) a->bad[g] = 1u;   // (the search must find the request that owns e)
            typename G::Point pm, pz;
            const uint32_t good = verify ? gq::element<G, true>(pm, pz, *a, g, e) : gq::element<G, false>(pm, pz, *a, g, e);
            if (!good) a->bad[g] = 1u;
            M = O::add(M, pm);
            if (verify) Z = O::add(Z, pz);
        }
        const uint32_t good = (cnt >= 1 && cnt <= gq::kMaxBatch && !a->bad[g]) ? 1u : 0u;
        if (!good) M = Z = O::identity();
        if (verify) gq::verify_tail<G>(*a, g, M, Z, good);
        else gq::prove_tail<G>(*a, g, M, good);
    }
}

template <class G>
void item(int op, const gq::ItemArgs *a, uint64_t i) {
    switch (op) {
        case gq::kTweakServer: gq::PoprfItem<G, gq::kTweakServer>::run(*a, i); break;
        case gq::kTweakClient: gq::PoprfItem<G, gq::kTweakClient>::run(*a, i); break;
        case gq::kPoprfFinalize: gq::PoprfItem<G, gq::kPoprfFinalize>::run(*a, i); break;
        case gq::kPoprfFullEvaluate: gq::PoprfItem<G, gq::kPoprfFullEvaluate>::run(*a, i); break;
    }
}

}  // namespace

#define BY_CURVE(CALL) (curve == 256 ? CALL<oprf::P256> : CALL<oprf::P384>)

extern "C" {

uint64_t hs_nistp_dleq_request_of(int curve, const gq::Args *a, uint64_t e) { return BY_CURVE(gq::request_of)(*a, e); }
// the element function: m and z as 3 N words each (X || Y || Z); returns its verdict
int hs_nistp_dleq_element(int curve, int verify, const gq::Args *a, uint64_t g, uint64_t e, uint32_t *m, uint32_t *z) {
    return BY_CURVE(element)(verify, a, g, e, m, z);
}
void hs_nistp_dleq_call(int curve, int verify, const gq::Args *a) { BY_CURVE(call)(verify, a); }
void hs_nistp_poprf_item(int curve, int op, const gq::ItemArgs *a, uint64_t i) { BY_CURVE(item)(op, a, i); }

}  // extern "C"

#ifdef DLEQ_NISTP_HOSTSIM_MAIN
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
// exactly n bytes that begin at an ODD address: the block is n + 1 bytes and the first one is not ours
struct Odd {
    uint8_t *base, *p;
    size_t n;
    explicit Odd(size_t n, uint32_t seed = 0) : base(static_cast<uint8_t *>(malloc(n + 1))), p(base + 1), n(n) {
        for (size_t i = 0; i < n; i++) p[i] = seed ? (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24) : 0;
    }
    ~Odd() { free(base); }
    Odd(const Odd &) = delete;
};

int fail(const char *what, int curve) {
    printf("FAIL P-%d %s\n", curve, what);
    return 1;
}

// a small non-zero canonical scalar as a big-endian row of ns bytes held in words
void small_scalar(uint32_t *row, size_t ns, uint32_t v) {
    uint8_t *b = reinterpret_cast<uint8_t *>(row);
    memset(b, 0, ns);
    for (int i = 0; i < 4; i++) {
        b[ns - 1 - i] = (uint8_t)(v >> (8 * i));
        b[ns - 13 - i] = (uint8_t)((v * 2654435761u) >> (8 * i));
    }
}

template <class G>
void base_mul(uint8_t *row, const uint32_t *k_row) {
    typename G::Scalar k;
    G::sc_load(k, k_row);
    uint32_t enc[G::EW];
    G::encode(enc, G::mul(k, G::generator()));
    G::elem_store(row, enc, 1);
}
template <class G>
void elem_mul(uint8_t *row, const uint32_t *k_row, const uint8_t *elem) {
    typename G::Scalar k;
    G::sc_load(k, k_row);
    uint32_t enc[G::EW];
    typename G::Point p;
    G::elem_load(enc, elem);
    G::decode(p, enc);
    G::encode(enc, G::mul(k, p));
    G::elem_store(row, enc, 1);
}

template <class G>
int run_proofs(int curve) {
    constexpr size_t NE = G::NE, SW = G::NS / 4;
    const size_t n_req = 4;
    const uint64_t off[n_req + 1] = {0, 1, 3, 3, 8};   // requests of 1, 2, 0 and 5 pairs
    const size_t n = 8;
    Rows k(SW * n_req), r(SW * n_req), proofs(2 * SW * n_req), bad(n_req), s(SW);
    Odd kA(NE * n_req), B(NE * n), kB(NE * n);
    std::vector<uint64_t> offs(off, off + n_req + 1);
    std::vector<uint8_t> ok(n_req, 7);
    for (size_t g = 0; g < n_req; g++) {
        small_scalar(k.w + SW * g, G::NS, 3 + (uint32_t)g);
        small_scalar(r.w + SW * g, G::NS, 1000 + (uint32_t)g);
        base_mul<G>(kA.p + NE * g, k.w + SW * g);
    }
    for (size_t e = 0; e < n; e++) {
        size_t g = 0;
        while (off[g + 1] <= e) g++;
        small_scalar(s.w, G::NS, 77 + (uint32_t)e);
        base_mul<G>(B.p + NE * e, s.w);
        elem_mul<G>(kB.p + NE * e, k.w + SW * g, B.p + NE * e);
    }
    gq::Args a = {};
    a.off = offs.data(); a.off_div = 1;
    a.B = B.p; a.kB = kB.p; a.k = k.w; a.k_stride = SW; a.kA = kA.p; a.kA_stride = NE; a.r = r.w; a.proofs = proofs.w; a.ok = ok.data();
    a.bad = bad.w; a.n_req = n_req; a.n_elems = n; a.flags = gq::kNoIdentity;
    uint8_t *at = gq::put_label(a.tag, "HashToScalar-OPRFV1-");   // the tag of mode 1
    *at++ = 1;
    a.tag_len = (uint32_t)(gq::put_label(at, gq::Ops<G>::ctx_tail()) - a.tag);
    call<G>(0, &a);
    if (ok[0] != 1 || ok[1] != 1 || ok[2] != 0 || ok[3] != 1) return fail("prove: ok", curve);
    for (size_t j = 0; j < 2 * SW; j++)
        if (proofs.w[2 * SW * 2 + j]) return fail("the empty request's proof row is not zero", curve);
    std::vector<uint8_t> verdict(n_req, 7);
    a.ok = verdict.data();
    call<G>(1, &a);
    if (verdict[0] != 1 || verdict[1] != 1 || verdict[2] != 0 || verdict[3] != 1) return fail("verify: the verdicts", curve);
    // the same with byte offsets, as the host pipeline passes them
    for (auto &o : offs) o *= NE;
    a.off_div = (uint32_t)NE;
    call<G>(1, &a);
    if (verdict[0] != 1 || verdict[1] != 1 || verdict[2] != 0 || verdict[3] != 1) return fail("verify: byte offsets", curve);
    kB.p[NE * 5] ^= 1u;   // an element of the last request: the other y
    call<G>(1, &a);
    if (verdict[0] != 1 || verdict[1] != 1 || verdict[3] != 0) return fail("verify: a tampered element passed, or disturbed a neighbour", curve);
    return 0;
}

template <class G>
int run_poprf(int curve) {
    constexpr size_t NE = G::NE, SW = G::NS / 4, HW = G::NH / 4;
    const size_t n = 4;
    std::vector<uint64_t> in_off(n + 1, 0), info_off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        in_off[i + 1] = in_off[i] + (i == 0 ? 0 : 40 * i + 3);
        info_off[i + 1] = info_off[i] + 7 * i;
    }
    Odd in(in_off[n], 5), info(info_off[n], 9), pk(NE), tg(NE * n), tweaked(NE * n), blinded(NE * n), evaluated(NE * n);
    Rows sk(SW), t(SW * n), tinv(SW * n), blinds(SW * n), out(HW * n), full(HW * n);
    std::vector<uint8_t> ok(n);
    small_scalar(sk.w, G::NS, 12345);
    base_mul<G>(pk.p, sk.w);
    gq::ItemArgs a = {};
    a.info = info.p; a.info_off = info_off.data(); a.scalars = sk.w; a.scalar_stride = 0;
    a.out = reinterpret_cast<uint8_t *>(t.w); a.out2 = reinterpret_cast<uint8_t *>(tinv.w); a.out3 = tg.p; a.ok = ok.data(); a.n = n;
    for (size_t i = 0; i < n; i++) { item<G>(gq::kTweakServer, &a, i); if (!ok[i]) return fail("tweak (server) refused an item", curve); }
    a.scalars = nullptr; a.elems = pk.p; a.elem_stride = 0; a.out = tweaked.p; a.out2 = a.out3 = nullptr;
    for (size_t i = 0; i < n; i++) { item<G>(gq::kTweakClient, &a, i); if (!ok[i]) return fail("tweak (client) refused an item", curve); }
    if (memcmp(tg.p, tweaked.p, NE * n)) return fail("t G != m G + pkS", curve);
    // blind, evaluate with t^-1 (base-mode items of oprf_group_kernels.h), finalize with the info; and the same in one step
    for (size_t i = 0; i < n; i++) small_scalar(blinds.w + SW * i, G::NS, 500 + (uint32_t)i);
    oprf::Args o = {};
    o.blob = in.p; o.off = in_off.data(); o.scalars = blinds.w; o.scalar_stride = SW; o.out = blinded.p; o.ok = ok.data(); o.n = n;
    o.dst_len = gq::mode2_tag<G>(o.dst, true);
    for (size_t i = 0; i < n; i++) { oprf::Item<G, oprf::kBlind, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("blind refused an item", curve); }
    o.blob = nullptr; o.off = nullptr; o.scalars = tinv.w; o.elems = blinded.p; o.out = evaluated.p;
    for (size_t i = 0; i < n; i++) { oprf::Item<G, oprf::kEvaluate, oprf::WAVES>::run(o, i); if (!ok[i]) return fail("evaluate refused an item", curve); }
    a.input = in.p; a.input_off = in_off.data(); a.scalars = blinds.w; a.scalar_stride = SW; a.elems = evaluated.p; a.elem_stride = NE;
    a.out = reinterpret_cast<uint8_t *>(out.w);
    for (size_t i = 0; i < n; i++) { item<G>(gq::kPoprfFinalize, &a, i); if (!ok[i]) return fail("poprf_finalize refused an item", curve); }
    a.scalars = sk.w; a.scalar_stride = 0; a.elems = nullptr; a.out = reinterpret_cast<uint8_t *>(full.w);
    for (size_t i = 0; i < n; i++) { item<G>(gq::kPoprfFullEvaluate, &a, i); if (!ok[i]) return fail("poprf_full_evaluate refused an item", curve); }
    if (memcmp(out.w, full.w, 4 * HW * n)) return fail("poprf_finalize(evaluate(blind(x))) != poprf_full_evaluate(x)", curve);
    return 0;
}

}  // namespace

int main() {
    const int bad = run_proofs<oprf::P256>(256) | run_poprf<oprf::P256>(256) | run_proofs<oprf::P384>(384) | run_poprf<oprf::P384>(384);
    puts(bad ? "dleq_nistp_hostsim: FAILED" : "dleq_nistp_hostsim: ok");
    return bad;
}
#endif
