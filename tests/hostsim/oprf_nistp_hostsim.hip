// tests/hostsim/oprf_nistp_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/nistp_dev.h and oprf_group_kernels.h on the CPU (their host instantiation), so that the CPU-only test tier can check the
// very source the P-256 / P-384 kernels are built from against the checker tests/oprf_nistp.py.
// Nothing here is linked into libcirclhip.so.
//
// Values cross this boundary as the ABI's rows: field elements and scalars as NS big-endian bytes, elements as NE bytes (in buffers
// of whole words).  With -DOPRF_NISTP_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: the same case classes checked
// by algebraic identities, and ragged batches whose blobs are heap blocks of exactly their size through every item function.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

// Only the host side of this file is ever run, and it is compiled host-only: plain inline instead of the device's forced inlining.
#define CIRCL_HD __host__ __device__ inline

#include "oprf_group_kernels.h"

using namespace circl;
using namespace circl::nistp;
using oprf::Args;
using oprf::WAVES;

namespace {

template <class C>
struct Sim {
    using Fp = typename C::Fp;
    using Fn = typename C::Fn;
    using F = Fe<C::N>;
    static constexpr int EW = elem_words<C>();

    static F fp_in(const uint32_t *row) { return to_mont<Fp>(sc_load<C>(row)); }
    static void fp_out(uint32_t *row, const F &x) { sc_store<C>(row, from_mont<Fp>(x), 1); }

    static void fe_mul(uint32_t *out, const uint32_t *a, const uint32_t *b) { fp_out(out, mont_mul<Fp>(fp_in(a), fp_in(b))); }
    static void fe_sqr(uint32_t *out, const uint32_t *a) { fp_out(out, mont_sqr<Fp>(fp_in(a))); }
    static void fe_inv_(uint32_t *out, const uint32_t *a) { fp_out(out, fe_inv<C>(fp_in(a))); }
    static int fe_sqrt(uint32_t *out, const uint32_t *a) {
        const F x = fp_in(a), y = fe_sqrt_candidate<C>(x);
        fp_out(out, y);
        return fe_equal(mont_sqr<Fp>(y), x);
    }
    static void fe_addsub(uint32_t *sum, uint32_t *diff, const uint32_t *a, const uint32_t *b) {
        fp_out(sum, fe_add<Fp>(fp_in(a), fp_in(b)));
        fp_out(diff, fe_sub<Fp>(fp_in(a), fp_in(b)));
    }
    static void reduce(int mod_n, uint32_t *out, const uint32_t *wide) {
        if (mod_n) sc_store<C>(out, from_mont<Fn>(reduce_wide<C, Fn>(wide, 0)), 1);
        else fp_out(out, reduce_wide<C, Fp>(wide, 0));
    }
    // the row prefix || x for a plain x of N limbs (any value below 2^(32 N))
    static void put_x(uint32_t *enc, const F &x, uint32_t prefix) {
        uint8_t *b = reinterpret_cast<uint8_t *>(enc);
        for (int j = 0; j < 4 * EW; j++) b[j] = 0;
        b[0] = (uint8_t)prefix;
        for (int j = 0; j < C::NS; j++) b[1 + j] = (uint8_t)(x.v[(C::NS - 1 - j) / 4] >> (8 * ((C::NS - 1 - j) % 4)));
    }
    static void map(uint32_t *enc, const uint32_t *u) { nistp_encode<C>(enc, sswu_map<C>(fp_in(u))); }
    static int decode_encode(uint32_t *out, const uint32_t *in) {
        Pt<C> p;
        const uint32_t good = nistp_decode<C>(p, in);
        nistp_encode<C>(out, p);
        return (int)good;
    }
    static int add(uint32_t *out, const uint32_t *a, const uint32_t *b) {
        Pt<C> p, q;
        const uint32_t good = nistp_decode<C>(p, a) & nistp_decode<C>(q, b);
        nistp_encode<C>(out, pt_add<C>(p, q));
        return (int)good;
    }
    static int dbl(uint32_t *out, const uint32_t *a) {
        Pt<C> p;
        const uint32_t good = nistp_decode<C>(p, a);
        nistp_encode<C>(out, pt_dbl<C>(p));
        return (int)good;
    }
    static int mul(uint32_t *out, const uint32_t *k, const uint32_t *elem) {
        Pt<C> p = pt_generator<C>();
        const uint32_t good = elem ? nistp_decode<C>(p, elem) : 1u;
        nistp_encode<C>(out, nistp_mul<C>(sc_load<C>(k), p));
        return (int)good;
    }
    static void sc_mul_(uint32_t *out, const uint32_t *a, const uint32_t *b) { sc_store<C>(out, sc_mul<C>(sc_load<C>(a), sc_load<C>(b)), 1); }
    static void sc_inv_(uint32_t *out, const uint32_t *a) { sc_store<C>(out, sc_inv<C>(sc_load<C>(a)), 1); }
    static int sc_canonical(const uint32_t *a) { return (int)sc_is_canonical<C>(sc_load<C>(a)); }
    static void xmd_(uint32_t *out, uint32_t out_len, const uint8_t *pre, uint32_t pre_len, const uint8_t *body, uint64_t body_len, const uint8_t *suf,
                     uint32_t suf_len, const uint8_t *dst, uint32_t dst_len) {
        hkdf::xmd<typename C::Hash, WAVES>(out, out_len, pre, pre_len, body, body_len, suf, suf_len, dst, dst_len);
    }
    static void item(int op, const Args *a, uint64_t i) {
        switch (op) {
            case oprf::kHashToGroup: oprf::Item<oprf::Nistp<C>, oprf::kHashToGroup, WAVES>::run(*a, i); break;
            case oprf::kHashToScalar: oprf::Item<oprf::Nistp<C>, oprf::kHashToScalar, WAVES>::run(*a, i); break;
            case oprf::kScalarMult: oprf::Item<oprf::Nistp<C>, oprf::kScalarMult, WAVES>::run(*a, i); break;
            case oprf::kDeriveKeyPair: oprf::Item<oprf::Nistp<C>, oprf::kDeriveKeyPair, WAVES>::run(*a, i); break;
            case oprf::kBlind: oprf::Item<oprf::Nistp<C>, oprf::kBlind, WAVES>::run(*a, i); break;
            case oprf::kEvaluate: oprf::Item<oprf::Nistp<C>, oprf::kEvaluate, WAVES>::run(*a, i); break;
            case oprf::kFinalize: oprf::Item<oprf::Nistp<C>, oprf::kFinalize, WAVES>::run(*a, i); break;
            case oprf::kFullEvaluate: oprf::Item<oprf::Nistp<C>, oprf::kFullEvaluate, WAVES>::run(*a, i); break;
        }
    }
};

}  // namespace

#define BY_CURVE(CALL) (curve == 256 ? Sim<P256>::CALL : Sim<P384>::CALL)

extern "C" {

void hs_fe_mul(int curve, uint32_t *out, const uint32_t *a, const uint32_t *b) { BY_CURVE(fe_mul(out, a, b)); }
void hs_fe_sqr(int curve, uint32_t *out, const uint32_t *a) { BY_CURVE(fe_sqr(out, a)); }
void hs_fe_inv(int curve, uint32_t *out, const uint32_t *a) { BY_CURVE(fe_inv_(out, a)); }
int hs_fe_sqrt(int curve, uint32_t *out, const uint32_t *a) { return BY_CURVE(fe_sqrt(out, a)); }
void hs_fe_addsub(int curve, uint32_t *sum, uint32_t *diff, const uint32_t *a, const uint32_t *b) { BY_CURVE(fe_addsub(sum, diff, a, b)); }
// the L-byte big-endian string modulo p, modulo n
void hs_reduce_wide_p(int curve, uint32_t *out, const uint32_t *wide) { BY_CURVE(reduce(0, out, wide)); }
void hs_reduce_wide_n(int curve, uint32_t *out, const uint32_t *wide) { BY_CURVE(reduce(1, out, wide)); }
void hs_map(int curve, uint32_t *enc, const uint32_t *u) { BY_CURVE(map(enc, u)); }
// out = encode(decode(in)) (computed whatever the verdict); returns decode's verdict
int hs_decode_encode(int curve, uint32_t *out, const uint32_t *in) { return BY_CURVE(decode_encode(out, in)); }
int hs_add(int curve, uint32_t *out, const uint32_t *a, const uint32_t *b) { return BY_CURVE(add(out, a, b)); }
int hs_dbl(int curve, uint32_t *out, const uint32_t *a) { return BY_CURVE(dbl(out, a)); }
// out = encode(k decode(elem)), elem NULL: the generator; returns decode's verdict
int hs_mul(int curve, uint32_t *out, const uint32_t *k, const uint32_t *elem) { return BY_CURVE(mul(out, k, elem)); }
void hs_sc_mul(int curve, uint32_t *out, const uint32_t *a, const uint32_t *b) { BY_CURVE(sc_mul_(out, a, b)); }
void hs_sc_inv(int curve, uint32_t *out, const uint32_t *a) { BY_CURVE(sc_inv_(out, a)); }
int hs_sc_is_canonical(int curve, const uint32_t *a) { return BY_CURVE(sc_canonical(a)); }
void hs_xmd(int curve, uint32_t *out, uint32_t out_len, const uint8_t *pre, uint32_t pre_len, const uint8_t *body, uint64_t body_len, const uint8_t *suf,
            uint32_t suf_len, const uint8_t *dst, uint32_t dst_len) {
    BY_CURVE(xmd_(out, out_len, pre, pre_len, body, body_len, suf, suf_len, dst, dst_len));
}
void hs_item(int curve, int op, const Args *a, uint64_t i) { BY_CURVE(item(op, a, i)); }

}  // extern "C"

#ifdef OPRF_NISTP_HOSTSIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// a ragged array whose blob is a heap block of exactly its size (so that a sanitizer sees any read past a row's end)
struct Rag {
    uint8_t *blob = nullptr;
    std::vector<uint64_t> off;
    Rag(size_t n, size_t (*len)(size_t), uint32_t seed) : off(n + 1, 0) {
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + len(i);
        blob = static_cast<uint8_t *>(malloc(off[n] ? off[n] : 1));
        for (uint64_t k = 0; k < off[n]; k++) blob[k] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    }
    ~Rag() { free(blob); }
    Rag(const Rag &) = delete;
};

// exact-size rows of bytes (malloc aligns them for word access)
struct Rows {
    uint8_t *b;
    size_t size;
    explicit Rows(size_t bytes) : b(static_cast<uint8_t *>(calloc(bytes ? bytes : 1, 1))), size(bytes) {}
    ~Rows() { free(b); }
    Rows(const Rows &) = delete;
    uint32_t *w() { return reinterpret_cast<uint32_t *>(b); }
};

int fail(int curve, const char *what) {
    printf("FAIL P-%d %s\n", curve, what);
    return 1;
}

template <class C>
struct Check {
    using S = Sim<C>;
    using Fp = typename C::Fp;
    using Fn = typename C::Fn;
    using F = Fe<C::N>;
    static constexpr int N = C::N, EW = elem_words<C>();
    uint32_t seed = 4242 + C::CURVE;

    uint32_t next() { return seed = seed * 1664525u + 1013904223u; }
    F random_below_p() {  // a random value with the top limb cleared is below either prime
        F x;
        for (int i = 0; i < N; i++) x.v[i] = next();
        x.v[N - 1] >>= 1;
        return x;
    }
    static F small(uint32_t k) {
        F x = fe_zero<Fp>();
        x.v[0] = k;
        return x;
    }
    static F mod_minus(uint32_t (*word)(int), uint32_t k) {  // the modulus minus a small k (no borrow leaves the low limb)
        F x;
        for (int i = 0; i < N; i++) x.v[i] = word(i);
        x.v[0] -= k;
        return x;
    }
    static bool same_point(const Pt<C> &p, const Pt<C> &q) {
        uint32_t a[EW], b[EW];
        nistp_encode<C>(a, p);
        nistp_encode<C>(b, q);
        return memcmp(a, b, sizeof a) == 0;
    }

    int field() {
        std::vector<F> xs = {small(0), small(1), small(2), mod_minus(Fp::mod, 1), mod_minus(Fp::mod, 2)};
        F ones;
        for (int i = 0; i < N; i++) ones.v[i] = i == N - 1 ? 0x7fffffffu : 0xffffffffu;
        xs.push_back(ones);
        for (int i = 0; i < 200; i++) xs.push_back(random_below_p());
        const F one = fe_one<Fp>();
        for (const F &plain : xs) {
            const F x = to_mont<Fp>(plain);
            if (!fe_equal(from_mont<Fp>(x), plain)) return fail(C::CURVE, "from_mont(to_mont(x)) != x");
            if (!fe_is_canonical<Fp>(x)) return fail(C::CURVE, "a product is not reduced");
            const F inv = fe_inv<C>(x), sq = mont_sqr<Fp>(x);
            if (!fe_equal(mont_mul<Fp>(x, inv), fe_is_zero(plain) ? fe_zero<Fp>() : one)) return fail(C::CURVE, "x x^-1 != 1");
            const F root = fe_sqrt_candidate<C>(sq);
            if (!fe_equal(mont_sqr<Fp>(root), sq)) return fail(C::CURVE, "sqrt(x^2)^2 != x^2");
            if (!fe_equal(root, x) && !fe_equal(root, fe_neg<Fp>(x))) return fail(C::CURVE, "sqrt(x^2) != +-x");
            if (!fe_equal(fe_sub<Fp>(fe_add<Fp>(x, sq), sq), x)) return fail(C::CURVE, "(x + y) - y != x");
            if (!fe_is_zero(fe_add<Fp>(x, fe_neg<Fp>(x)))) return fail(C::CURVE, "x + (-x) != 0");
        }
        // scalars
        for (const F &k : {small(1), small(2), mod_minus(Fn::mod, 1), mod_minus(Fn::mod, 2), random_below_p()}) {
            if (!sc_is_canonical<C>(k)) return fail(C::CURVE, "a scalar below n is refused");
            if (!fe_equal(sc_mul<C>(k, sc_inv<C>(k)), small(1))) return fail(C::CURVE, "k k^-1 != 1 mod n");
        }
        if (sc_is_canonical<C>(mod_minus(Fn::mod, 0)) || !fe_is_zero(sc_inv<C>(small(0)))) return fail(C::CURVE, "n is canonical, or 0^-1 != 0");
        return 0;
    }

    int wide() {
        constexpr int W = C::L / 4;
        uint32_t u[W];
        for (int i = 0; i < W; i++) u[i] = 0;
        if (!fe_is_zero(reduce_wide<C, Fp>(u, 0)) || !fe_is_zero(reduce_wide<C, Fn>(u, 0))) return fail(C::CURVE, "0 mod m != 0");
        for (int i = 0; i < W; i++) u[i] = 0xffffffffu;
        // 2^(8 L) - 1 = (2^(8 L) mod m) - 1, and 2^(8 L) = R 2^(8 L - 32 N): check against a product of powers of two
        F two = fe_zero<Fp>();
        two.v[(8 * C::L - 32 * N) / 32] = 1u << ((8 * C::L - 32 * N) % 32);
        const F wantp = fe_sub<Fp>(mont_mul<Fp>(to_mont<Fp>(fe_lit<Fp>(Fp::one)), to_mont<Fp>(two)), fe_one<Fp>());
        if (!fe_equal(reduce_wide<C, Fp>(u, 0), wantp)) return fail(C::CURVE, "2^(8 L) - 1 mod p");
        const F wantn = fe_sub<Fn>(mont_mul<Fn>(to_mont<Fn>(fe_lit<Fn>(Fn::one)), to_mont<Fn>(two)), fe_one<Fn>());
        if (!fe_equal(reduce_wide<C, Fn>(u, 0), wantn)) return fail(C::CURVE, "2^(8 L) - 1 mod n");
        return 0;
    }

    int points() {
        const Pt<C> g = pt_generator<C>(), e = pt_identity<C>();
        uint32_t enc[EW], back[EW];
        // k G for k = 0 .. 16 against repeated addition; the encoding decodes back to itself
        Pt<C> acc = e;
        for (uint32_t k = 0; k <= 16; k++) {
            if (!same_point(nistp_mul<C>(small(k), g), acc)) return fail(C::CURVE, "k G != G + ... + G");
            nistp_encode<C>(enc, acc);
            Pt<C> p;
            if (!nistp_decode<C>(p, enc)) return fail(C::CURVE, "k G does not decode");
            nistp_encode<C>(back, p);
            if (memcmp(enc, back, sizeof enc)) return fail(C::CURVE, "encode(decode(x)) != x");
            acc = pt_add<C>(acc, g);
        }
        // the complete addition: P + P, P + (-P), P + identity, identity + identity
        const Pt<C> neg_g = {g.X, fe_neg<Fp>(g.Y), g.Z};
        if (!same_point(pt_add<C>(g, g), pt_dbl<C>(g))) return fail(C::CURVE, "P + P != 2 P");
        if (!pt_is_identity<C>(pt_add<C>(g, neg_g))) return fail(C::CURVE, "P + (-P) != identity");
        if (!same_point(pt_add<C>(g, e), g) || !same_point(pt_add<C>(e, g), g)) return fail(C::CURVE, "P + identity != P");
        if (!pt_is_identity<C>(pt_add<C>(e, e)) || !pt_is_identity<C>(pt_dbl<C>(e))) return fail(C::CURVE, "identity + identity != identity");
        // (n - 1) G = -G, (n - 2) G + 2 G = identity, 2 ((n + 1) / 2) G = G
        if (!same_point(nistp_mul<C>(mod_minus(Fn::mod, 1), g), neg_g)) return fail(C::CURVE, "(n - 1) G != -G");
        if (!pt_is_identity<C>(pt_add<C>(nistp_mul<C>(mod_minus(Fn::mod, 2), g), pt_dbl<C>(g)))) return fail(C::CURVE, "(n - 2) G + 2 G != identity");
        F half = mod_minus(Fn::mod, 0);  // (n + 1) / 2 = (n >> 1) + 1: n is odd
        for (int i = 0; i < N; i++) half.v[i] = (half.v[i] >> 1) | (i + 1 < N ? half.v[i + 1] << 31 : 0u);
        half.v[0] += 1;  // (the low limb of n >> 1 is not all ones for either order)
        if (!same_point(pt_dbl<C>(nistp_mul<C>(half, g)), g)) return fail(C::CURVE, "2 ((n + 1) / 2) G != G");
        // the map: u = 0 and random u land on the curve (the encoding decodes)
        for (int i = 0; i < 12; i++) {
            const F u = i == 0 ? fe_zero<Fp>() : to_mont<Fp>(random_below_p());
            nistp_encode<C>(enc, sswu_map<C>(u));
            Pt<C> p;
            if (!nistp_decode<C>(p, enc) || (enc[0] & 0xfe) != 2) return fail(C::CURVE, "map_to_curve left the curve");
        }
        // strict decoding: x = p, p + 1, all ones; prefixes 00, 04, 05 on a good x; a non-residue x
        nistp_encode<C>(enc, g);
        for (uint32_t prefix : {0u, 4u, 5u}) {
            memcpy(back, enc, sizeof enc);
            back[0] = (back[0] & ~0xffu) | prefix;
            Pt<C> p;
            if (nistp_decode<C>(p, back)) return fail(C::CURVE, "a bad prefix decodes");
        }
        F over[3] = {mod_minus(Fp::mod, 0), mod_minus(Fp::mod, 0), mod_minus(Fp::mod, 0)};  // p, p + 1, 2^(8 NS) - 1
        for (int i = 0, carry = 1; i < N; i++) {
            over[1].v[i] += (uint32_t)carry;
            carry = carry && over[1].v[i] == 0;
            over[2].v[i] = 0xffffffffu;
        }
        for (const F &x : over) {
            S::put_x(back, x, 2);
            Pt<C> p;
            if (nistp_decode<C>(p, back)) return fail(C::CURVE, "x >= p decodes");
        }
        int refused = 0;
        for (uint32_t x = 0; x < 16; x++) {  // about half of these small x are non-residues: each decodes exactly when its rhs is a square
            S::put_x(back, small(x), 2);
            Pt<C> p;
            const uint32_t good = nistp_decode<C>(p, back);
            const F xm = to_mont<Fp>(small(x));
            const F rhs = fe_add<Fp>(fe_sub<Fp>(mont_mul<Fp>(mont_sqr<Fp>(xm), xm), fe_add<Fp>(fe_add<Fp>(xm, xm), xm)), fe_lit<Fp>(C::b));
            const F y = fe_sqrt_candidate<C>(rhs);
            if (good != (fe_equal(mont_sqr<Fp>(y), rhs) ? 1u : 0u)) return fail(C::CURVE, "decode's verdict is not the residue test");
            refused += !good;
        }
        if (refused == 0 || refused == 16) return fail(C::CURVE, "no non-residue (or no residue) among the small x");
        return 0;
    }

    static void set_dst(Args &a, const char *label, int mode) {
        size_t at = 0;
        for (const char *s = label; *s; s++) a.dst[at++] = (uint8_t)*s;
        for (const char *s = "OPRFV1-"; *s; s++) a.dst[at++] = (uint8_t)*s;
        a.dst[at++] = (uint8_t)mode;
        for (const char *s = C::CURVE == 256 ? "-P256-SHA256" : "-P384-SHA384"; *s; s++) a.dst[at++] = (uint8_t)*s;
        a.dst_len = (uint32_t)at;
    }

    int run(int mode) {
        const size_t n = 6;
        constexpr size_t NS = C::NS, NE = C::NE, NH = C::Hash::OUT;
        // lengths on both sides of the padding edges of the xmd and the Finalize message of both hashes
        Rag in(n, [](size_t i) { static const size_t L[] = {0, 1, 19, 20, 83, 300}; return L[i % 6]; }, 11 + mode);
        Rag info(n, [](size_t i) { return i * 3; }, 5);
        Rows seeds(32 * n), sk(NS * n), pk(NE * n), blinds(NS * n), blinded(NE * n), evaluated(NE * n), out(NH * n), full(NH * n), unblinded(NE * n);
        std::vector<uint8_t> ok(n);
        for (size_t j = 0; j < 32 * n; j++) seeds.b[j] = (uint8_t)(next() >> 24);
        Args a = {};
        a.n = n;
        a.ok = ok.data();
        a.blob = info.blob; a.off = info.off.data(); a.seeds = seeds.w(); a.out = sk.b; a.out2 = pk.b;
        set_dst(a, "DeriveKeyPair", mode);
        for (size_t i = 0; i < n; i++) { S::item(oprf::kDeriveKeyPair, &a, i); if (!ok[i]) return fail(C::CURVE, "derive_keypair refused an item"); }
        // blinds: any non-zero canonical scalars; the keys serve
        for (size_t i = 0; i < n; i++) memcpy(blinds.b + NS * i, sk.b + NS * ((i + 1) % n), NS);
        a.blob = in.blob; a.off = in.off.data(); a.scalars = blinds.w(); a.scalar_stride = N; a.out = blinded.b; a.out2 = nullptr;
        set_dst(a, "HashToGroup-", mode);
        for (size_t i = 0; i < n; i++) { S::item(oprf::kBlind, &a, i); if (!ok[i]) return fail(C::CURVE, "blind refused an item"); }
        // evaluate under the shared key sk[0], finalize, and the same in one step
        a.blob = nullptr; a.off = nullptr; a.scalars = sk.w(); a.scalar_stride = 0; a.elems = blinded.b; a.out = evaluated.b;
        for (size_t i = 0; i < n; i++) { S::item(oprf::kEvaluate, &a, i); if (!ok[i]) return fail(C::CURVE, "evaluate refused an item"); }
        a.blob = in.blob; a.off = in.off.data(); a.scalars = blinds.w(); a.scalar_stride = N; a.elems = evaluated.b; a.out = out.b;
        for (size_t i = 0; i < n; i++) { S::item(oprf::kFinalize, &a, i); if (!ok[i]) return fail(C::CURVE, "finalize refused an item"); }
        a.scalars = sk.w(); a.scalar_stride = 0; a.elems = nullptr; a.out = full.b;
        for (size_t i = 0; i < n; i++) { S::item(oprf::kFullEvaluate, &a, i); if (!ok[i]) return fail(C::CURVE, "full_evaluate refused an item"); }
        if (memcmp(out.b, full.b, NH * n)) return fail(C::CURVE, "finalize(evaluate(blind(x))) != full_evaluate(x)");
        // scalar_mult by the inverse undoes a blinding: blind^-1 (blind P) = P = hash_to_group(x)
        a.blob = nullptr; a.off = nullptr; a.scalars = blinds.w(); a.scalar_stride = N; a.elems = blinded.b; a.out = unblinded.b; a.flags = 1;
        for (size_t i = 0; i < n; i++) { S::item(oprf::kScalarMult, &a, i); if (!ok[i]) return fail(C::CURVE, "scalar_mult refused an item"); }
        a.flags = 0; a.blob = in.blob; a.off = in.off.data(); a.out = evaluated.b;
        for (size_t i = 0; i < n; i++) S::item(oprf::kHashToGroup, &a, i);
        if (memcmp(unblinded.b, evaluated.b, NE * n)) return fail(C::CURVE, "blind^-1 (blind P) != P");
        a.flags = 1;
        for (size_t i = 0; i < n; i++) S::item(oprf::kHashToGroup, &a, i);
        a.flags = 0; a.out = sk.b;
        for (size_t i = 0; i < n; i++) S::item(oprf::kHashToScalar, &a, i);
        // failure masks: a zero blind, an element that does not decode
        memset(blinds.b, 0, NS);
        blinded.b[NE] = 4;
        a.scalars = blinds.w(); a.scalar_stride = N; a.out = unblinded.b;
        S::item(oprf::kBlind, &a, 0);
        a.scalars = sk.w(); a.scalar_stride = 0; a.elems = blinded.b;
        S::item(oprf::kEvaluate, &a, 1);
        for (size_t j = 0; j < 2 * NE; j++)
            if (unblinded.b[j]) return fail(C::CURVE, "a failed item's row is not zero");
        if (ok[0] || ok[1]) return fail(C::CURVE, "a bad blind or element passed");
        return 0;
    }

    int xmd_lengths() {
        // the byte-ragged hash at every length across two blocks of either hash, on exact-size blocks and with tags of 1, 31 and 255 bytes
        for (uint32_t dl : {1u, 31u, 255u})
            for (size_t len = 0; len <= 140; len++) {
                uint8_t *m = static_cast<uint8_t *>(malloc(len ? len : 1)), *d = static_cast<uint8_t *>(malloc(dl));
                memset(m, (int)len, len);
                memset(d, 0x44, dl);
                uint32_t o[uniform_words<C, 2>()];
                S::xmd_(o, 2 * C::L, m, (uint32_t)(len / 3), m + len / 3, len - len / 3, nullptr, 0, d, dl);
                S::xmd_(o, C::L, nullptr, 0, m, len, nullptr, 0, d, dl);
                free(m);
                free(d);
            }
        return 0;
    }

    int all() {
        int bad = field() | wide() | points() | xmd_lengths();
        for (int mode = 0; mode < 3; mode++) bad |= run(mode);
        return bad;
    }
};

}  // namespace

int main() {
    const int bad = Check<P256>().all() | Check<P384>().all();
    puts(bad ? "oprf_nistp_hostsim: FAILED" : "oprf_nistp_hostsim: ok");
    return bad;
}
#endif
