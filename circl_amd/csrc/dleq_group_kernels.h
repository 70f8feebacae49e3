// dleq_group_kernels.h -- batch DLEQ proofs (zk/dleq with Params{G, H, DST}, the ...RFC9497 forms: fixed generator, the base not bound;
// RFC 9497 section 2.2) and the mode-2 (POPRF) item operations of oprf/client.go and oprf/server.go, written once over a group
// description G of oprf_group_kernels.h.  Instantiated for R255 (api_dleq.hip) and for P256 and P384 (api_dleq_nistp.hip); beyond that
// description it asks of a group what Ops<G> below lists.
//
// A proof belongs to a REQUEST: a ragged group of 1 .. 65535 element pairs (B_j, kB_j).  Two launches per call:
//   composite<G, VERIFY>  one lane per ELEMENT.  The lane finds its request by an upper-bound search over the offsets (empty requests
//                         are skipped), recomputes the request's seed, hashes d_j and multiplies: d_j B_j, and d_j kB_j when verifying.
//                         Then a segmented reduction inside the wavefront: six __shfl_down steps over the PW words of a point (40 for
//                         ristretto255, 24 for P-256, 36 for P-384) and the request index; a lane adds what it received only if the
//                         sender exists and is of the same request.  Requests are contiguous, so the first lane of every request
//                         segment of the wave ends up with the segment's sum, and writes it to
//                         workspace slot (wave + request): unique and increasing along the (wave, request) pairs, at most
//                         ceil(n_elems / 64) + n_req slots.  Every lane reaches every shuffle: a lane beyond n_elems or with a failed
//                         element carries the identity (the addition formulas are complete), and a failed element raises the request's
//                         flag in the workspace.
//   finish<G, VERIFY>     one lane per REQUEST: adds the request's slots (contiguous, at most 1025) and runs the prover's or verifier's
//                         tail.  kA is decoded here, once per request, not once per element.
// d_j and the elements are public; the prover's k M, r M, r G and s = r - c k act on secrets and use the constant-time routines.  Nothing
// secret reaches the workspace.  The hashes and the tails' multiplications are functions of their own (noinline); the other
// multiplications and the additions are too where Ops<G>::CALLS says so; k times the generator is the group's fixed-base routine where
// it has one (base_mul).
//
//   element rows   are addressed as the group addresses them (oprf::elem_rows<G>, G::ROW): words for ristretto255, packed unaligned
//                  bytes for the NIST curves; kA and pkS too, and their strides are BYTES for every group.
//   offsets        the host pipeline's blobs carry BYTE offsets, and 33 and 49 are no powers of two, so a shift cannot scale them.
//                  Args::off_div is a DIVISOR: 1 where the offsets count elements (the _dev forms), G::NE where they count bytes (the
//                  host pipeline's chunks).  The kernels compare it with those two values only, so the division is by a constant.
#pragma once
#include <hip/hip_runtime.h>

#include "oprf_group_kernels.h"

namespace circl {
namespace gdleq {

using oprf::store_masked;
using oprf::wipe;

constexpr int WAVES = oprf::WAVES;
constexpr uint64_t kMaxBatch = 0xffff;   // the index j travels as two bytes
constexpr uint32_t kNoIdentity = 1u;     // flags bit 0
constexpr int kTagHead = 13;             // "HashToScalar-"

// What the proofs ask of a group beyond oprf_group_kernels.h's description: the group law on two public or secret points, a point as
// words, the scalar field's sum and r - c k, and the suite's name as the group description spells it (G::ctx_tail()).
template <class G>
struct Ops;
template <>
struct Ops<oprf::R255> {
    using Ge = ed25519::Ge;
    using Scalar = oprf::R255::Scalar;
    static constexpr int PW = 40;
    static constexpr bool CALLS = false;
    static CIRCL_HD Ge identity() { return ed25519::ge_identity(); }
    static CIRCL_HD Ge add(const Ge &p, const Ge &q) { return r255::r255_add(p, q); }
    static CIRCL_HD void store(uint32_t *w, const Ge &p) {
#pragma unroll
        for (int i = 0; i < 10; i++) {
            w[i] = p.X.v[i];
            w[10 + i] = p.Y.v[i];
            w[20 + i] = p.Z.v[i];
            w[30 + i] = p.T.v[i];
        }
    }
    static CIRCL_HD Ge load(const uint32_t *w) {
        Ge p;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            p.X.v[i] = w[i];
            p.Y.v[i] = w[10 + i];
            p.Z.v[i] = w[20 + i];
            p.T.v[i] = w[30 + i];
        }
        return p;
    }
    static CIRCL_HD void sc_add(Scalar &out, const Scalar &a, const Scalar &b) {
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        ed25519::sc_muladd(out, a, one, b);
    }
    // r - c k mod L, for c below L: (L - c) k + r (c = 0 gives L, which the product reduces)
    static CIRCL_HD void sc_sub_mul(Scalar &out, const Scalar &r, const Scalar &c, const Scalar &k) {
        uint32_t nc[8];
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint64_t t = (uint64_t)ed25519::order_word(i) - c[i] - borrow;
            nc[i] = (uint32_t)t;
            borrow = (t >> 32) & 1u;
        }
        ed25519::sc_muladd(out, nc, k, r);
    }
    static CIRCL_HD bool sc_equal(const Scalar &a, const Scalar &b) { return ed25519::words_equal(a, b); }
    static CIRCL_HD const char *ctx_tail() { return oprf::R255::ctx_tail(); }
};
template <class C>
struct Ops<oprf::Nistp<C>> {
    using G = oprf::Nistp<C>;
    static constexpr int PW = 3 * C::N;   // words of a point in a lane's hands and in the workspace
    static constexpr bool CALLS = true;   // mul() and add() below
    static CIRCL_HD typename G::Point identity() { return nistp::pt_identity<C>(); }
    static CIRCL_HD typename G::Point add(const typename G::Point &p, const typename G::Point &q) { return nistp::pt_add<C>(p, q); }
    static CIRCL_HD void store(uint32_t *w, const typename G::Point &p) { nistp::pt_store<C>(w, p); }
    static CIRCL_HD typename G::Point load(const uint32_t *w) { return nistp::pt_load<C>(w); }
    static CIRCL_HD void sc_add(typename G::Scalar &out, const typename G::Scalar &a, const typename G::Scalar &b) { out = nistp::fe_add<typename C::Fn>(a, b); }
    // r - c k mod n, for c below n
    static CIRCL_HD void sc_sub_mul(typename G::Scalar &out, const typename G::Scalar &r, const typename G::Scalar &c, const typename G::Scalar &k) {
        out = nistp::fe_sub<typename C::Fn>(r, nistp::sc_mul<C>(c, k));
    }
    static CIRCL_HD bool sc_equal(const typename G::Scalar &a, const typename G::Scalar &b) { return nistp::fe_equal(a, b); }
    static CIRCL_HD const char *ctx_tail() { return G::ctx_tail(); }
};

struct Args {
    const uint64_t *off;       // n_req + 1 offsets, in elements times off_div
    uint32_t off_div;          // 1, or G::NE (the host pipeline's byte offsets)
    const uint8_t *B, *kB;     // element rows (oprf::elem_rows<G>), indexed by the ABSOLUTE element index off[g] / off_div
    const uint32_t *k;         // prove: rows of NS / 4 words, k_stride words apart (0: one key for the call)
    size_t k_stride;
    const uint8_t *kA;         // element rows, kA_stride BYTES apart (0: one key for the call)
    size_t kA_stride;
    const uint32_t *r;         // prove: rows of NS / 4 words
    uint32_t *proofs;          // rows of NS / 2 words, c || s: prove writes them, verify reads them
    uint8_t *ok;               // prove: may be nullptr
    uint32_t *partial;         // workspace: slots of PW (prove) or 2 PW (verify) words
    uint32_t *bad;             // workspace: one word per request, zero before composite runs
    size_t n_req, n_elems;
    uint32_t flags, tag_len;
    uint8_t tag[256];          // "HashToScalar-" || dst; "Seed-" || dst is made from its tail
};

template <class G>
CIRCL_HD uint64_t elem_off(const Args &a, size_t g) { return a.off_div == 1 ? a.off[g] : a.off[g] / (uint64_t)G::NE; }

// the request of absolute element e, off[0] <= e < off[n_req]: the LAST g with off[g] <= e, so that empty requests are skipped
template <class G>
CIRCL_HD size_t request_of(const Args &a, uint64_t e) {
    size_t lo = 0, hi = a.n_req;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (elem_off<G>(a, mid) <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

CIRCL_HD uint8_t *put_i2(uint8_t *m, uint32_t v) {
    m[0] = (uint8_t)(v >> 8);
    m[1] = (uint8_t)v;
    return m + 2;
}
CIRCL_HD uint8_t *put_bytes(uint8_t *m, const uint32_t *w, int bytes) {
    for (int i = 0; i < bytes; i++) m[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    return m + bytes;
}
CIRCL_HD uint8_t *put_label(uint8_t *m, const char *s) {
    for (; *s; s++) *m++ = (uint8_t)*s;
    return m;
}

// seed = H(I2(Ne) || kA || I2(len("Seed-" || dst)) || "Seed-" || dst): NH / 4 words
template <class G, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void seed_hash(uint32_t *seed, const uint32_t *kA, const uint8_t *tag, uint32_t tag_len) {
    hkdf::Stream<typename G::Hash, WV> st;
    const uint32_t ctx_len = tag_len - kTagHead, dst_len = 5 + ctx_len;
    st.init();
    st.put((uint8_t)0);
    st.put((uint8_t)G::NE);
    st.put(reinterpret_cast<const uint8_t *>(kA), G::NE);
    st.put((uint8_t)(dst_len >> 8));
    st.put((uint8_t)dst_len);
    const char label[] = "Seed-";
    for (int j = 0; j < 5; j++) st.put((uint8_t)label[j]);
    st.put(tag + kTagHead, ctx_len);
    st.finish(seed);
}

// d_j = HashToScalar(I2(Nh) || seed || I2(j) || I2(Ne) || B_j || I2(Ne) || kB_j || "Composite", tag)
template <class G>
CIRCL_HD void composite_scalar(typename G::Scalar &d, const uint32_t *seed, uint32_t j, const uint32_t *b, const uint32_t *kb, const uint8_t *tag,
                               uint32_t tag_len) {
    constexpr int LEN = 2 + G::NH + 2 + 2 * (2 + G::NE) + 9;
    uint8_t m[LEN];
    uint32_t u[oprf::uniform_words<G>(G::LEN_SCALAR)];
    uint8_t *at = put_bytes(put_i2(m, G::NH), seed, G::NH);
    at = put_i2(at, j);
    at = put_bytes(put_i2(at, G::NE), b, G::NE);
    at = put_bytes(put_i2(at, G::NE), kb, G::NE);
    put_label(at, "Composite");
    hkdf::xmd<typename G::Hash, WAVES>(u, G::LEN_SCALAR, m, LEN, nullptr, 0, nullptr, 0, tag, tag_len);
    G::sc_from_uniform(d, u);
}

// c = HashToScalar(I2(Ne) || kA || I2(Ne) || M || I2(Ne) || Z || I2(Ne) || t2 || I2(Ne) || t3 || "Challenge", tag); rows = the five encodings
template <class G>
CIRCL_HD void challenge_scalar(typename G::Scalar &c, const uint32_t *rows, const uint8_t *tag, uint32_t tag_len) {
    constexpr int LEN = 5 * (2 + G::NE) + 9;
    uint8_t m[LEN];
    uint32_t u[oprf::uniform_words<G>(G::LEN_SCALAR)];
    uint8_t *at = m;
    for (int e = 0; e < 5; e++) at = put_bytes(put_i2(at, G::NE), rows + G::EW * e, G::NE);
    put_label(at, "Challenge");
    hkdf::xmd<typename G::Hash, WAVES>(u, G::LEN_SCALAR, m, LEN, nullptr, 0, nullptr, 0, tag, tag_len);
    G::sc_from_uniform(c, u);
    for (int i = 0; i < LEN; i++) m[i] = 0;   // (the prover's Z and t3 are derived from secrets)
    wipe<oprf::uniform_words<G>(G::LEN_SCALAR)>(u);
}

// k P as a call: composite multiplies once or twice and the tails three or four times, and one copy of the loop keeps its registers
template <class G, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void mul_call(typename G::Point &out, const typename G::Scalar &k, const typename G::Point &p) {
    out = G::mul(k, p);
}
// P + Q as a call: the shuffle loop, the slot loop and the verifier's tail add in six places
template <class G, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void add_call(typename G::Point &out, const typename G::Point &p, const typename G::Point &q) {
    out = Ops<G>::add(p, q);
}
// k P and P + Q outside the tails, as Ops<G>::CALLS says: through the calls above (the NIST curves, whose kernels would not hold a second
// copy of either), or in line (ristretto255: its composite multiplies once or twice and adds in the shuffle loop; as calls the points
// cross by address and composite's scratch grows by 400 and 608 bytes per lane, profiles/dleq_fold_static.txt)
template <class G>
CIRCL_HD void mul(typename G::Point &out, const typename G::Scalar &k, const typename G::Point &p) {
    if constexpr (Ops<G>::CALLS) mul_call<G, WAVES>(out, k, p);
    else out = G::mul(k, p);
}
template <class G>
CIRCL_HD void add(typename G::Point &out, const typename G::Point &p, const typename G::Point &q) {
    if constexpr (Ops<G>::CALLS) add_call<G, WAVES>(out, p, q);
    else out = Ops<G>::add(p, q);
}
// k times the generator: the group's fixed-base routine (FIXED_BASE: ristretto255's comb), or the one multiplication run on generator()
template <class G>
CIRCL_HD void base_mul(typename G::Point &out, const typename G::Scalar &k) {
    if constexpr (G::FIXED_BASE) {
        out = G::base(k);
    } else {
        const typename G::Point gen = G::generator();
        mul_call<G, WAVES>(out, k, gen);
    }
}

// The lane-local part of composite: m = d_j B_j and, when verifying, z = d_j kB_j for absolute element e of request g.  Returns 0
// (and identities) where the request cannot be proven: more than 65535 pairs, an element that does not decode, an identity element
// under kNoIdentity.  kA is hashed here and decoded by the tail.  Everything here is public.
template <class G, bool VERIFY>
CIRCL_HD uint32_t element(typename G::Point &m, typename G::Point &z, const Args &a, size_t g, uint64_t e) {
    const uint64_t first = elem_off<G>(a, g), cnt = elem_off<G>(a, g + 1) - first;
    uint32_t ka[G::EW], b[G::EW], kb[G::EW], seed[G::NH / 4], ib, ikb;
    G::elem_load(ka, oprf::elem_rows<G>(a.kA + g * a.kA_stride));
    G::elem_load(b, oprf::elem_rows<G>(a.B) + (size_t)G::ROW * e);
    G::elem_load(kb, oprf::elem_rows<G>(a.kB) + (size_t)G::ROW * e);
    typename G::Point pb, pkb;
    uint32_t good = (cnt <= kMaxBatch ? 1u : 0u) & G::decode(pb, b, &ib) & G::decode(pkb, kb, &ikb);
    if (a.flags & kNoIdentity) good &= (ib | ikb) ^ 1u;
    m = Ops<G>::identity();
    z = Ops<G>::identity();
    if (!good) return 0;
    typename G::Scalar d;
    seed_hash<G, WAVES>(seed, ka, a.tag, a.tag_len);
    composite_scalar<G>(d, seed, (uint32_t)(e - first), b, kb, a.tag, a.tag_len);
    mul<G>(m, d, pb);
    if (VERIFY) mul<G>(z, d, pkb);
    return 1;
}

// The prover's tail for request g on its composite M: Z = k M, t2 = r G, t3 = r M, c, s = r - c k.  k and r are secrets.
template <class G>
CIRCL_HD void prove_tail(const Args &a, size_t g, const typename G::Point &M, uint32_t good) {
    constexpr int SW = G::NS / 4;
    uint32_t rows[5 * G::EW];
    typename G::Scalar k, r, c, s;
    G::sc_load(k, a.k + g * a.k_stride);
    G::sc_load(r, a.r + (size_t)SW * g);
    G::elem_load(rows, oprf::elem_rows<G>(a.kA + g * a.kA_stride));
    typename G::Point p;
    good &= oprf::secret_scalar_ok<G>(k) & oprf::secret_scalar_ok<G>(r) & G::decode(p, rows);
    mul_call<G, WAVES>(p, k, M);
    G::encode(rows + G::EW, M);
    G::encode(rows + 2 * G::EW, p);
    base_mul<G>(p, r);
    G::encode(rows + 3 * G::EW, p);
    mul_call<G, WAVES>(p, r, M);
    G::encode(rows + 4 * G::EW, p);
    challenge_scalar<G>(c, rows, a.tag, a.tag_len);
    Ops<G>::sc_sub_mul(s, r, c, k);
    G::sc_store(a.proofs + (size_t)2 * SW * g, c, good);
    G::sc_store(a.proofs + (size_t)2 * SW * g + SW, s, good);
    if (a.ok) a.ok[g] = (uint8_t)good;
    G::wipe(k);
    G::wipe(r);
    G::wipe(s);
    wipe<5 * G::EW>(rows);
    G::wipe(p);
}

// The verifier's tail for request g on its composites M and Z: t2 = s G + c kA, t3 = s M + c Z; the verdict is "the recomputed c equals c"
template <class G>
CIRCL_HD void verify_tail(const Args &a, size_t g, const typename G::Point &M, const typename G::Point &Z, uint32_t good) {
    constexpr int SW = G::NS / 4;
    uint32_t rows[5 * G::EW];
    typename G::Scalar c, s, c2;
    G::sc_load(c, a.proofs + (size_t)2 * SW * g);
    G::sc_load(s, a.proofs + (size_t)2 * SW * g + SW);
    G::elem_load(rows, oprf::elem_rows<G>(a.kA + g * a.kA_stride));
    typename G::Point pa, t, u;
    good &= G::sc_is_canonical(c) & G::sc_is_canonical(s) & G::decode(pa, rows);
    G::encode(rows + G::EW, M);
    G::encode(rows + 2 * G::EW, Z);
    mul_call<G, WAVES>(u, c, pa);
    base_mul<G>(t, s);
    add<G>(t, t, u);
    G::encode(rows + 3 * G::EW, t);
    mul_call<G, WAVES>(t, s, M);
    mul_call<G, WAVES>(u, c, Z);
    add<G>(t, t, u);
    G::encode(rows + 4 * G::EW, t);
    challenge_scalar<G>(c2, rows, a.tag, a.tag_len);
    good &= Ops<G>::sc_equal(c2, c) ? 1u : 0u;
    a.ok[g] = (uint8_t)good;
}

template <class G, bool VERIFY>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void composite(const Args a) {
    constexpr int PW = Ops<G>::PW;
    const size_t lane_e = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = lane_e < a.n_elems;
    unsigned long long g = a.n_req;   // of no request: a lane beyond the elements never joins a live lane's sum
    uint32_t mw[PW], zw[PW];
    {
        typename G::Point m = Ops<G>::identity(), z = Ops<G>::identity();
        if (live) {
            const uint64_t e = elem_off<G>(a, 0) + lane_e;
            g = request_of<G>(a, e);
            if (!element<G, VERIFY>(m, z, a, (size_t)g, e)) a.bad[g] = 1u;
        }
        Ops<G>::store(mw, m);
        if (VERIFY) Ops<G>::store(zw, z);
    }
    // the segmented reduction: every lane of the wave takes every shuffle
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const unsigned long long g2 = __shfl_down(g, d);
        uint32_t rw[PW];
#pragma unroll
        for (int i = 0; i < PW; i++) rw[i] = __shfl_down(mw[i], d);
        const bool take = threadIdx.x + d < 64 && g2 == g;
        if (take) {
            typename G::Point s;
            add<G>(s, Ops<G>::load(mw), Ops<G>::load(rw));
            Ops<G>::store(mw, s);
        }
        if (VERIFY) {
#pragma unroll
            for (int i = 0; i < PW; i++) rw[i] = __shfl_down(zw[i], d);
            if (take) {
                typename G::Point s;
                add<G>(s, Ops<G>::load(zw), Ops<G>::load(rw));
                Ops<G>::store(zw, s);
            }
        }
    }
    const unsigned long long g_prev = __shfl_up(g, 1);
    if (!live || (threadIdx.x != 0 && g_prev == g)) return;   // not the first lane of a request's segment in this wave
    uint32_t *slot = a.partial + ((size_t)blockIdx.x + (size_t)g) * (VERIFY ? 2 * PW : PW);
#pragma unroll
    for (int i = 0; i < PW; i++) slot[i] = mw[i];
    if (VERIFY) {
#pragma unroll
        for (int i = 0; i < PW; i++) slot[PW + i] = zw[i];
    }
}

template <class G, bool VERIFY>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void finish(const Args a) {
    constexpr int PW = Ops<G>::PW;
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= a.n_req) return;
    const uint64_t first = elem_off<G>(a, g) - elem_off<G>(a, 0), cnt = elem_off<G>(a, g + 1) - elem_off<G>(a, g);
    const uint32_t good = (cnt >= 1 && cnt <= kMaxBatch && first + cnt <= a.n_elems && !a.bad[g]) ? 1u : 0u;   // (n_elems: the slots that exist)
    typename G::Point M = Ops<G>::identity(), Z = Ops<G>::identity();
    if (good) {
        const size_t w1 = (size_t)((first + cnt - 1) / 64);
#pragma unroll 1
        for (size_t w = (size_t)(first / 64); w <= w1; w++) {
            const uint32_t *slot = a.partial + (w + g) * (VERIFY ? 2 * PW : PW);
            add<G>(M, M, Ops<G>::load(slot));
            if (VERIFY) add<G>(Z, Z, Ops<G>::load(slot + PW));
        }
    }
    if (VERIFY) verify_tail<G>(a, g, M, Z, good);
    else prove_tail<G>(a, g, M, good);
}

// ---- mode 2 (POPRF): oprf/server.go secretFromInfo, client.go pointFromInfo, and the Finalize / FullEvaluate that hash the info -------
enum ItemOp : int { kTweakServer = 0, kTweakClient, kPoprfFinalize, kPoprfFullEvaluate, kItemOps };

struct ItemArgs {
    const uint8_t *input;      // the ragged inputs (finalize, full_evaluate); nullptr: every item's is empty
    const uint64_t *input_off;
    const uint8_t *info;       // the ragged infos; nullptr: every item's is empty
    const uint64_t *info_off;
    const uint32_t *scalars;   // sk (tweak server, full_evaluate; scalar_stride words apart, 0: one key) or blinds (finalize)
    size_t scalar_stride;
    const uint8_t *elems;      // pkS (tweak client; elem_stride BYTES apart, 0: one key) or evaluated elements (finalize): element rows
    size_t elem_stride;
    uint8_t *out, *out2, *out3;   // tweak server: t, t^-1 (words), t G (an element row); tweak client: the tweaked key; finalize / full_evaluate: NH / 4 words
    uint8_t *ok;               // may be nullptr
    size_t n;
};

CIRCL_HD uint64_t rag(const uint8_t *&p, const uint8_t *blob, const uint64_t *off, size_t i) {
    if (!blob || !off) {
        p = nullptr;
        return 0;
    }
    p = blob + off[i];
    return off[i + 1] - off[i];
}

// "HashToScalar-" || "OPRFV1-" || 2 || the suite's name, or "HashToGroup-" || the same; at most 48 bytes
template <class G>
CIRCL_HD uint32_t mode2_tag(uint8_t *tag, bool to_group) {
    uint8_t *at = put_label(tag, to_group ? "HashToGroup-OPRFV1-" : "HashToScalar-OPRFV1-");
    *at++ = 2;
    at = put_label(at, Ops<G>::ctx_tail());
    return (uint32_t)(at - tag);
}

// m = HashToScalar("Info" || I2(len) || info, "HashToScalar-" || ctx_2)
template <class G>
CIRCL_HD void info_scalar(typename G::Scalar &m, const uint8_t *info, uint64_t len) {
    uint8_t tag[48], pre[6] = {'I', 'n', 'f', 'o', (uint8_t)(len >> 8), (uint8_t)len};
    uint32_t u[oprf::uniform_words<G>(G::LEN_SCALAR)];
    const uint32_t tag_len = mode2_tag<G>(tag, false);
    hkdf::xmd<typename G::Hash, WAVES>(u, G::LEN_SCALAR, pre, 6, info, len, nullptr, 0, tag, tag_len);
    G::sc_from_uniform(m, u);
}

// H(I2(len) || input || I2(len) || info || I2(Ne) || element || "Finalize")
template <class G, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void finalize_hash2(uint32_t *out, const uint8_t *input, uint64_t len, const uint8_t *info, uint64_t info_len, const uint32_t *element) {
    hkdf::Stream<typename G::Hash, WV> st;
    st.init();
    st.put((uint8_t)(len >> 8));
    st.put((uint8_t)len);
    st.put(input, len);
    st.put((uint8_t)(info_len >> 8));
    st.put((uint8_t)info_len);
    st.put(info, info_len);
    st.put((uint8_t)0);
    st.put((uint8_t)G::NE);
    st.put(reinterpret_cast<const uint8_t *>(element), G::NE);
    const char tag[] = "Finalize";
    for (int j = 0; j < 8; j++) st.put((uint8_t)tag[j]);
    st.finish(out);
}

// t = sk + m, and verdict 0 where sk is no key, the info is too long or t = 0 (ErrInverseZero)
template <class G>
CIRCL_HD uint32_t tweaked_secret(typename G::Scalar &t, const ItemArgs &a, size_t i, const uint8_t *info, uint64_t info_len) {
    const bool fits = info_len <= oprf::kMaxInputBytes;
    typename G::Scalar sk, m;
    G::sc_load(sk, a.scalars + i * a.scalar_stride);
    info_scalar<G>(m, info, fits ? info_len : 0);
    Ops<G>::sc_add(t, sk, m);
    const uint32_t good = oprf::secret_scalar_ok<G>(sk) & (fits ? 1u : 0u) & (G::sc_is_zero(t) ? 0u : 1u);
    G::wipe(sk);
    return good;
}

template <class G, int OP>
struct PoprfItem;

template <class G>
struct PoprfItem<G, kTweakServer> {
    static CIRCL_HD void run(const ItemArgs &a, size_t i) {
        constexpr int SW = G::NS / 4;
        const uint8_t *info;
        const uint64_t info_len = rag(info, a.info, a.info_off, i);
        uint32_t enc[G::EW];
        typename G::Scalar t, tinv;
        const uint32_t good = tweaked_secret<G>(t, a, i, info, info_len);
        G::sc_inv(tinv, t);
        typename G::Point p;
        base_mul<G>(p, t);
        G::encode(enc, p);
        G::sc_store(oprf::word_rows(a.out) + (size_t)SW * i, t, good);
        G::sc_store(oprf::word_rows(a.out2) + (size_t)SW * i, tinv, good);
        G::elem_store(oprf::elem_rows<G>(a.out3) + (size_t)G::ROW * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        G::wipe(t);
        G::wipe(tinv);
        G::wipe(p);
    }
};

template <class G>
struct PoprfItem<G, kTweakClient> {
    static CIRCL_HD void run(const ItemArgs &a, size_t i) {
        const uint8_t *info;
        const uint64_t info_len = rag(info, a.info, a.info_off, i);
        const bool fits = info_len <= oprf::kMaxInputBytes;
        uint32_t enc[G::EW];
        typename G::Scalar m;
        G::elem_load(enc, oprf::elem_rows<G>(a.elems + i * a.elem_stride));
        typename G::Point p, q;
        uint32_t good = G::decode(p, enc) & (fits ? 1u : 0u);
        info_scalar<G>(m, info, fits ? info_len : 0);
        base_mul<G>(q, m);
        add<G>(p, q, p);
        good &= G::encode(enc, p) ^ 1u;   // the tweaked key is the identity
        G::elem_store(oprf::elem_rows<G>(a.out) + (size_t)G::ROW * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
    }
};

template <class G>
struct PoprfItem<G, kPoprfFinalize> {
    static CIRCL_HD void run(const ItemArgs &a, size_t i) {
        constexpr int HW = G::NH / 4;
        const uint8_t *m, *info;
        const uint64_t len = rag(m, a.input, a.input_off, i), info_len = rag(info, a.info, a.info_off, i);
        const bool fits = len <= oprf::kMaxInputBytes && info_len <= oprf::kMaxInputBytes;
        uint32_t enc[G::EW], h[HW], ident;
        typename G::Scalar k, kinv;
        G::sc_load(k, a.scalars + i * a.scalar_stride);
        G::elem_load(enc, oprf::elem_rows<G>(a.elems) + (size_t)G::ROW * i);
        typename G::Point p;
        uint32_t good = oprf::secret_scalar_ok<G>(k) & G::decode(p, enc, &ident) & (fits ? 1u : 0u);
        good &= ident ^ 1u;
        G::sc_inv(kinv, k);
        mul<G>(p, kinv, p);
        G::encode(enc, p);
        finalize_hash2<G, WAVES>(h, m, fits ? len : 0, info, fits ? info_len : 0, enc);
        store_masked<HW>(oprf::word_rows(a.out) + (size_t)HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        G::wipe(k);
        G::wipe(kinv);
        wipe<G::EW>(enc);
        wipe<HW>(h);
        G::wipe(p);
    }
};

template <class G>
struct PoprfItem<G, kPoprfFullEvaluate> {
    static CIRCL_HD void run(const ItemArgs &a, size_t i) {
        constexpr int HW = G::NH / 4, UW = oprf::uniform_words<G>(G::LEN_ELEM);
        const uint8_t *m, *info;
        const uint64_t len = rag(m, a.input, a.input_off, i), info_len = rag(info, a.info, a.info_off, i);
        const bool fits = len <= oprf::kMaxInputBytes;
        uint8_t tag[48];
        uint32_t u[UW], enc[G::EW], h[HW];
        typename G::Scalar t, tinv;
        uint32_t good = tweaked_secret<G>(t, a, i, info, info_len) & (fits ? 1u : 0u);
        G::sc_inv(tinv, t);
        const uint32_t tag_len = mode2_tag<G>(tag, true);
        hkdf::xmd<typename G::Hash, WAVES>(u, G::LEN_ELEM, nullptr, 0, m, fits ? len : 0, nullptr, 0, tag, tag_len);
        typename G::Point p = G::from_uniform(u, false);
        mul<G>(p, tinv, p);
        good &= G::encode(enc, p) ^ 1u;   // the hashed point was the identity
        finalize_hash2<G, WAVES>(h, m, fits ? len : 0, info, info_len <= oprf::kMaxInputBytes ? info_len : 0, enc);
        store_masked<HW>(oprf::word_rows(a.out) + (size_t)HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<UW>(u);
        G::wipe(t);
        G::wipe(tinv);
        wipe<G::EW>(enc);
        wipe<HW>(h);
        G::wipe(p);
    }
};

template <class G, int OP>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void item_kernel(const ItemArgs a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    PoprfItem<G, OP>::run(a, i);
}

}  // namespace gdleq
}  // namespace circl
