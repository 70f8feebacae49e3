// oprf_group_kernels.h -- batch prime-order group operations (group/ristretto255.go, group/short.go) and the proof-free part of OPRF
// (RFC 9497; oprf/keys.go, oprf/client.go, oprf/server.go), written once over a group description G: one item per lane, one launch per
// call, no workspace.  Three groups: R255 (ristretto255-SHA512, on ristretto255_dev.h / ed25519_dev.h), P256 and P384 (P256-SHA256 and
// P384-SHA384, on the curve descriptions of nistp_dev.h).
//
// One item function per public operation (Item<G, OP, WV>::run), one kernel per item function and group.  expand_message_xmd and the
// Finalize hash are functions of their own (hkdf::xmd, finalize_hash), so that the field loops of the multiplication keep their register
// allocation and what a hash holds does not live across them; each is instantiated for the occupancy class of the kernels (WAVES).  A
// hashed point, an evaluated element before it is hashed, a blind's inverse: none of them reaches memory.
//
// Failure is a mask: ok[i] = 0 and every output row of item i is zero.  The verdicts are computed without a branch on a secret; only
// lengths (public) and the launch-wide flags steer control flow.  Secrets a lane held are zeroed before it returns.
//
// What a group description supplies -- exactly what the items use:
//   Scalar, Point, Hash        the lane's types and the suite's hash
//   NS, NE, NH                 bytes of a scalar row, an element row, an OPRF output; EW: the words an element row takes in registers
//   Row, ROW                   what element rows are addressed by in memory -- words (R255) or bytes (the NIST curves) -- and how many of
//                              them a row is.  alignof(Row) is the alignment the host layer asks of an element pointer: 4 or 1
//   LEN_SCALAR, LEN_ELEM, LEN_ELEM_NU   the uniform bytes of hash_to_scalar, hash_to_group and its non-uniform form
//   sc_load / sc_store         a scalar row (words, 4-byte aligned) <-> Scalar; the store is masked
//   sc_is_canonical / sc_is_zero / sc_inv / sc_from_uniform   results through a reference (R255's Scalar is a bare array); sc_inv may work in place
//   elem_load / elem_store     an element row <-> EW words; the store is masked
//   decode(p, enc, &ident)     the verdict, the point (computed either way), and whether the row is the identity's
//   encode(enc, p)             the row; returns 1 for the identity.  R255 tests the encoding, the NIST curves their Z coordinate
//   mul(k, p)                  k P for a secret k and a secret P
//   FIXED_BASE                 base(k) is a routine of its own (R255's comb) and scalar_mult without elements uses it; otherwise
//                              generator() supplies the point and the one multiplication runs on it (the NIST curves)
//   base(k)                    k times the generator
//   from_uniform(u, nonuniform)
//   ctx_tail()                 the end of the suite's context string, its name: the one place that spells it
//   wipe(Scalar &), wipe(Point &)
//
// Rows: scalars, keys and blinds are NS bytes read as words; seeds are 32 bytes and OPRF outputs NH bytes, words too; elements are packed
// rows of NE bytes.  R255 is 32 / 32 / 64 little-endian, P256 32 / 33 / 32 and P384 48 / 49 / 48 big-endian.
//
// What the compiler reports for gfx950 (-Rpass-analysis=kernel-resource-usage; WAVES = 2 allows 256 registers), VGPRs / scratch bytes
// per lane, occupancy 2 waves per SIMD for every kernel: profiles/oprf_group_fold_static.txt, kernel by kernel against the two headers
// this one replaced.  P-256's field loops use no scratch (what the hashing kernels report is the hash streams' buffers, passed by
// address).  P-384's twelve-limb points do NOT fit 256 registers: the bare multiplication spills 208 bytes (52 words) per lane, the
// kernels that also decode or hash more.  Correctness and constant time were not traded for registers.
#pragma once
#include <hip/hip_runtime.h>

#include "nistp_dev.h"
#include "ristretto255_dev.h"

namespace circl {
namespace oprf {

constexpr int WAVES = 2;  // the Ed25519 kernels' class: two points and a product's temporaries in 256 registers
constexpr uint64_t kMaxInputBytes = 0xffff;  // RFC 9497: inputs and infos carry a two-byte length

enum Op : int { kHashToGroup = 0, kHashToScalar, kScalarMult, kDeriveKeyPair, kBlind, kEvaluate, kFinalize, kFullEvaluate, kOps };

struct Args {
    const uint8_t *blob;       // the ragged argument (messages, infos, inputs); nullptr: every item's is empty
    const uint64_t *off;
    const uint32_t *scalars;   // rows of NS / 4 words, scalar_stride words apart (0: one row for the batch): scalars, keys, blinds
    size_t scalar_stride;
    const uint8_t *elems;      // rows of NE bytes: elements, blinded / evaluated elements; nullptr (kScalarMult): the generator
    const uint32_t *seeds;     // kDeriveKeyPair: rows of 8 words
    uint8_t *out;              // rows of NE bytes (elements), of NS / 4 words (kHashToScalar, kDeriveKeyPair: sk) or of NH / 4 words (outputs)
    uint8_t *out2;             // kDeriveKeyPair: the public keys, rows of NE bytes
    uint8_t *ok;               // may be nullptr
    uint32_t flags;            // kScalarMult: bit 0 = by the scalar's inverse; kHashToGroup: bit 0 = non-uniform (one map)
    uint32_t dst_len;
    size_t n;
    uint8_t dst[256];          // the domain separation tag of the launch's hash
};

CIRCL_HD uint64_t item_range(const uint8_t *&p, const Args &a, size_t i) {
    if (!a.blob || !a.off) {
        p = nullptr;
        return 0;
    }
    p = a.blob + a.off[i];
    return a.off[i + 1] - a.off[i];
}
CIRCL_HD void load8(uint32_t w[8], const uint32_t *p) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = p[j];
}
template <int N>
CIRCL_HD void store_masked(uint32_t *p, const uint32_t *w, uint32_t good) {
    const uint32_t mask = 0u - good;
#pragma unroll
    for (int j = 0; j < N; j++) p[j] = w[j] & mask;
}
template <int N>
CIRCL_HD void wipe(uint32_t *w) {
#pragma unroll
    for (int j = 0; j < N; j++) w[j] = 0;
}

// ---- ristretto255-SHA512: scalars and elements are eight little-endian words ---------------------------------------------------------
CIRCL_HD void wipe(ed25519::Ge &p) { p = ed25519::ge_identity(); }

struct R255 {
    using Scalar = uint32_t[8];  // (a bare array: wrapped in a struct the same words are allocated differently in scalar_mult)
    using Point = ed25519::Ge;
    using Hash = hkdf::Sha512;
    using Row = uint32_t;
    static constexpr int NS = 32, NE = 32, NH = 64, EW = 8, ROW = 8, LEN_SCALAR = 64, LEN_ELEM = 64, LEN_ELEM_NU = 64;
    static constexpr bool FIXED_BASE = true;

    static CIRCL_HD void sc_load(Scalar &k, const uint32_t *row) { load8(k, row); }
    static CIRCL_HD void sc_store(uint32_t *row, const Scalar &k, uint32_t good) { store_masked<8>(row, k, good); }
    static CIRCL_HD uint32_t sc_is_canonical(const Scalar &k) { return ed25519::sc_is_canonical(k); }
    static CIRCL_HD bool sc_is_zero(const Scalar &k) { return r255::sc_is_zero(k); }
    static CIRCL_HD void sc_inv(Scalar &out, const Scalar &k) { r255::sc_inv(out, k); }
    static CIRCL_HD void sc_from_uniform(Scalar &out, const uint32_t *u) { r255::sc_from_uniform(out, u); }
    static CIRCL_HD void elem_load(uint32_t *enc, const Row *row) { load8(enc, row); }
    static CIRCL_HD void elem_store(Row *row, const uint32_t *enc, uint32_t good) { store_masked<8>(row, enc, good); }
    static CIRCL_HD uint32_t decode(Point &p, const uint32_t *enc, uint32_t *ident = nullptr) {
        const uint32_t good = r255::r255_decode(p, enc);
        if (ident) *ident = r255::r255_equal_identity(enc) ? 1u : 0u;
        return good;
    }
    static CIRCL_HD uint32_t encode(uint32_t *enc, const Point &p) {
        r255::r255_encode(enc, p);
        return r255::r255_equal_identity(enc) ? 1u : 0u;
    }
    static CIRCL_HD Point mul(const Scalar &k, const Point &p) { return r255::r255_mul(k, p); }
    static CIRCL_HD Point base(const Scalar &k) { return r255::r255_base(k); }
    static CIRCL_HD Point from_uniform(const uint32_t *u, bool) { return r255::r255_from_uniform(u); }
    static constexpr CIRCL_HD const char *ctx_tail() { return "-ristretto255-SHA512"; }
    static CIRCL_HD void wipe(Scalar &k) { oprf::wipe<8>(k); }
    static CIRCL_HD void wipe(Point &p) { oprf::wipe(p); }
};

// ---- P256-SHA256 / P384-SHA384: scalars are big-endian rows read as words, elements SEC 1 compressed points read bytewise -------------
template <class C>
struct Nistp {
    using Scalar = nistp::Fe<C::N>;
    using Point = nistp::Pt<C>;
    using Hash = typename C::Hash;
    using Row = uint8_t;
    static constexpr int NS = C::NS, NE = C::NE, NH = Hash::OUT, EW = nistp::elem_words<C>(), ROW = C::NE, LEN_SCALAR = C::L, LEN_ELEM = 2 * C::L,
                         LEN_ELEM_NU = C::L;
    static constexpr bool FIXED_BASE = false;

    static CIRCL_HD void sc_load(Scalar &k, const uint32_t *row) { k = nistp::sc_load<C>(row); }
    static CIRCL_HD void sc_store(uint32_t *row, const Scalar &k, uint32_t good) { nistp::sc_store<C>(row, k, good); }
    static CIRCL_HD uint32_t sc_is_canonical(const Scalar &k) { return nistp::sc_is_canonical<C>(k); }
    static CIRCL_HD bool sc_is_zero(const Scalar &k) { return nistp::sc_is_zero<C>(k); }
    static CIRCL_HD void sc_inv(Scalar &out, const Scalar &k) { out = nistp::sc_inv<C>(k); }
    static CIRCL_HD void sc_from_uniform(Scalar &out, const uint32_t *u) { out = nistp::sc_from_uniform<C>(u); }
    static CIRCL_HD void elem_load(uint32_t *enc, const Row *row) { nistp::elem_load<C>(enc, row); }
    static CIRCL_HD void elem_store(Row *row, const uint32_t *enc, uint32_t good) { nistp::elem_store<C>(row, enc, good); }
    static CIRCL_HD uint32_t decode(Point &p, const uint32_t *enc, uint32_t *ident = nullptr) { return nistp::nistp_decode<C>(p, enc, ident); }
    static CIRCL_HD uint32_t encode(uint32_t *enc, const Point &p) { return nistp::nistp_encode<C>(enc, p); }
    static CIRCL_HD Point mul(const Scalar &k, const Point &p) { return nistp::nistp_mul<C>(k, p); }
    static CIRCL_HD Point base(const Scalar &k) { return nistp::nistp_base<C>(k); }
    static CIRCL_HD Point generator() { return nistp::pt_generator<C>(); }
    static CIRCL_HD Point from_uniform(const uint32_t *u, bool nonuniform) { return nistp::nistp_from_uniform<C>(u, nonuniform); }
    static constexpr CIRCL_HD const char *ctx_tail() { return C::CURVE == 256 ? "-P256-SHA256" : "-P384-SHA384"; }
    static CIRCL_HD void wipe(Scalar &k) { oprf::wipe<C::N>(k.v); }
    static CIRCL_HD void wipe(Point &p) {
        wipe(p.X);
        wipe(p.Y);
        wipe(p.Z);
    }
};
using P256 = Nistp<nistp::P256>;
using P384 = Nistp<nistp::P384>;

// what the host layers (oprf_host.h, dleq_host.h) read off a group description: a row per group
enum GroupId : int { kNoGroup = -1, kR255 = 0, kP256, kP384, kGroups };
struct Suite {
    size_t ns, ne, nh, elem_align;   // a scalar row, an element row, an OPRF output; what an element row's address must be a multiple of
    const char *ctx_tail;            // the end of the suite's context string
};
template <class G> constexpr Suite suite_of() { return {G::NS, G::NE, G::NH, alignof(typename G::Row), G::ctx_tail()}; }
constexpr Suite kSuites[kGroups] = {suite_of<R255>(), suite_of<P256>(), suite_of<P384>()};

// ---- the operations, once ---------------------------------------------------------------------------------------------------------------
// 1 for a scalar a key or a blind may be: canonical and not zero
template <class G>
CIRCL_HD uint32_t secret_scalar_ok(const typename G::Scalar &k) { return G::sc_is_canonical(k) & (G::sc_is_zero(k) ? 0u : 1u); }
// the words that hold an xmd of len bytes: whole digests
template <class G>
constexpr int uniform_words(int len) { return (len + G::Hash::OUT - 1) / G::Hash::OUT * (G::Hash::OUT / 4); }
// Args' byte pointers as the group addresses element rows, and as rows of words (scalars, OPRF outputs).  Casts only: an item computes a
// row's position itself, G::ROW * i or the words times i, next to its other uses.  Computed inside a helper the product has one use there
// and is folded into a byte offset before the helper is inlined; ristretto255's evaluate then keeps that offset in two more spilled
// registers across the multiplication.
template <class G>
CIRCL_HD const typename G::Row *elem_rows(const uint8_t *p) { return reinterpret_cast<const typename G::Row *>(p); }
template <class G>
CIRCL_HD typename G::Row *elem_rows(uint8_t *p) { return reinterpret_cast<typename G::Row *>(p); }
CIRCL_HD uint32_t *word_rows(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

// oprf/client.go Finalize / server.go FullEvaluate: H(I2OSP(len, 2) || input || I2OSP(NE, 2) || element || "Finalize")
template <class G, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void finalize_hash(uint32_t *out, const uint8_t *input, uint64_t len, const uint32_t *element) {
    hkdf::Stream<typename G::Hash, WV> st;
    st.init();
    st.put((uint8_t)(len >> 8));
    st.put((uint8_t)len);
    st.put(input, len);
    st.put((uint8_t)0);
    st.put((uint8_t)G::NE);
    st.put(reinterpret_cast<const uint8_t *>(element), G::NE);
    const char tag[] = "Finalize";
    for (int j = 0; j < 8; j++) st.put((uint8_t)tag[j]);
    st.finish(out);
}

template <class G, int OP, int WV>
struct Item;

// Group.HashToElement(msg, dst), or HashToElementNonUniform where flags & 1
template <class G, int WV>
struct Item<G, kHashToGroup, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool nu = (a.flags & 1u) != 0;  // (a launch-wide flag)
        uint32_t u[uniform_words<G>(G::LEN_ELEM)], enc[G::EW];
        hkdf::xmd<typename G::Hash, WV>(u, nu ? G::LEN_ELEM_NU : G::LEN_ELEM, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
        G::encode(enc, G::from_uniform(u, nu));
        G::elem_store(elem_rows<G>(a.out) + G::ROW * i, enc, 1);
    }
};

// Group.HashToScalar(msg, dst)
template <class G, int WV>
struct Item<G, kHashToScalar, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        uint32_t u[uniform_words<G>(G::LEN_SCALAR)];
        hkdf::xmd<typename G::Hash, WV>(u, G::LEN_SCALAR, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
        typename G::Scalar s;
        G::sc_from_uniform(s, u);
        G::sc_store(word_rows(a.out) + G::NS / 4 * i, s, 1);
    }
};

// Element.Mul / Element.MulGen, optionally by the scalar's inverse: the scalar below the order, the element any valid one (the identity too)
template <class G, int WV>
struct Item<G, kScalarMult, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        uint32_t enc[G::EW];
        typename G::Scalar k;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        uint32_t good = G::sc_is_canonical(k);
        if (a.flags & 1u) {  // (a launch-wide flag)
            good &= G::sc_is_zero(k) ? 0u : 1u;
            G::sc_inv(k, k);
        }
        // k times the element, or k times the generator: a fixed-base routine of its own (FIXED_BASE), or the one multiplication run on
        // generator() -- a second copy of its loop would double the kernel
        typename G::Point p;
        if (a.elems) {
            G::elem_load(enc, elem_rows<G>(a.elems) + G::ROW * i);
            good &= G::decode(p, enc);
            if constexpr (G::FIXED_BASE) p = G::mul(k, p);
        } else {
            if constexpr (G::FIXED_BASE) p = G::base(k);
            else p = G::generator();
        }
        if constexpr (!G::FIXED_BASE) p = G::mul(k, p);
        G::encode(enc, p);
        G::elem_store(elem_rows<G>(a.out) + G::ROW * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        G::wipe(k);
        G::wipe(p);
    }
};

// oprf/keys.go DeriveKey: sk = HashToScalar(seed || I2OSP(len(info), 2) || info || counter, "DeriveKeyPair" || ctx) for the first
// counter in 0..255 that gives a non-zero scalar, pk = sk G.  The loop ends on "the scalar is not zero": a scalar that the loop
// discards is never a key, and that a candidate was zero (probability 2^-252 or less each) says nothing about the one that is kept.
template <class G, int WV>
struct Item<G, kDeriveKeyPair, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *info;
        const uint64_t info_len = item_range(info, a, i);
        const bool fits = info_len <= kMaxInputBytes;
        uint32_t pre[9], u[uniform_words<G>(G::LEN_SCALAR)], pk[G::EW];
        load8(pre, a.seeds + 8 * i);
        pre[8] = (uint32_t)((info_len >> 8) & 0xff) | (uint32_t)(info_len & 0xff) << 8;
        uint32_t good = 0;
        typename G::Scalar sk;
        G::wipe(sk);
        for (uint32_t counter = 0; counter < 256 && !good; counter++) {
            const uint8_t c = (uint8_t)counter;
            hkdf::xmd<typename G::Hash, WV>(u, G::LEN_SCALAR, reinterpret_cast<const uint8_t *>(pre), 34, info, fits ? info_len : 0, &c, 1, a.dst, a.dst_len);
            G::sc_from_uniform(sk, u);
            good = G::sc_is_zero(sk) ? 0u : 1u;
        }
        good &= fits ? 1u : 0u;
        typename G::Point p = G::base(sk);
        G::encode(pk, p);
        G::sc_store(word_rows(a.out) + G::NS / 4 * i, sk, good);
        G::elem_store(elem_rows<G>(a.out2) + G::ROW * i, pk, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<9>(pre);
        wipe<uniform_words<G>(G::LEN_SCALAR)>(u);
        G::wipe(sk);
        G::wipe(p);
    }
};

// oprf/client.go DeterministicBlind: blinded = blind HashToGroup(input)
template <class G, int WV>
struct Item<G, kBlind, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t u[uniform_words<G>(G::LEN_ELEM)], enc[G::EW];
        typename G::Scalar k;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        uint32_t good = secret_scalar_ok<G>(k) & (fits ? 1u : 0u);
        hkdf::xmd<typename G::Hash, WV>(u, G::LEN_ELEM, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
        typename G::Point p = G::from_uniform(u, false);
        p = G::mul(k, p);
        // blind != 0 and the group has prime order: the blinded element is the identity exactly where the hashed point is
        good &= G::encode(enc, p) ^ 1u;
        G::elem_store(elem_rows<G>(a.out) + G::ROW * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<uniform_words<G>(G::LEN_ELEM)>(u);
        G::wipe(k);
        G::wipe(p);
    }
};

// oprf/server.go Server.Evaluate (base mode): evaluated = sk blinded
template <class G, int WV>
struct Item<G, kEvaluate, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        uint32_t enc[G::EW], ident;
        typename G::Scalar k;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        G::elem_load(enc, elem_rows<G>(a.elems) + G::ROW * i);
        typename G::Point p;
        uint32_t good = secret_scalar_ok<G>(k) & G::decode(p, enc, &ident);
        good &= ident ^ 1u;
        p = G::mul(k, p);
        G::encode(enc, p);
        G::elem_store(elem_rows<G>(a.out) + G::ROW * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        G::wipe(k);
        G::wipe(p);
    }
};

// oprf/client.go Client.Finalize (base mode): output = Hash(input, blind^-1 evaluated)
template <class G, int WV>
struct Item<G, kFinalize, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        constexpr int HW = G::NH / 4;
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t enc[G::EW], h[HW], ident;
        typename G::Scalar k;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        G::elem_load(enc, elem_rows<G>(a.elems) + G::ROW * i);
        typename G::Point p;
        uint32_t good = secret_scalar_ok<G>(k) & G::decode(p, enc, &ident) & (fits ? 1u : 0u);
        good &= ident ^ 1u;
        typename G::Scalar kinv;
        G::sc_inv(kinv, k);
        p = G::mul(kinv, p);
        G::encode(enc, p);
        finalize_hash<G, WV>(h, m, fits ? len : 0, enc);
        store_masked<HW>(word_rows(a.out) + HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        G::wipe(k);
        G::wipe(kinv);
        wipe<G::EW>(enc);
        wipe<HW>(h);
        G::wipe(p);
    }
};

// oprf/server.go Server.FullEvaluate / VerifiableServer.FullEvaluate: output = Hash(input, sk HashToGroup(input))
template <class G, int WV>
struct Item<G, kFullEvaluate, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        constexpr int HW = G::NH / 4;
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t u[uniform_words<G>(G::LEN_ELEM)], enc[G::EW], h[HW];
        typename G::Scalar k;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        uint32_t good = secret_scalar_ok<G>(k) & (fits ? 1u : 0u);
        hkdf::xmd<typename G::Hash, WV>(u, G::LEN_ELEM, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
        typename G::Point p = G::from_uniform(u, false);
        p = G::mul(k, p);
        good &= G::encode(enc, p) ^ 1u;  // as in kBlind: the hashed point was the identity
        finalize_hash<G, WV>(h, m, fits ? len : 0, enc);
        store_masked<HW>(word_rows(a.out) + HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<uniform_words<G>(G::LEN_ELEM)>(u);
        G::wipe(k);
        wipe<G::EW>(enc);
        wipe<HW>(h);
        G::wipe(p);
    }
};

template <class G, int OP>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    Item<G, OP, WAVES>::run(a, i);
}

}  // namespace oprf
}  // namespace circl
