// dleq_kernels.h -- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms: fixed generator, the base not bound; RFC 9497 section 2.2) on
// ristretto255, and the mode-2 (POPRF) item operations of oprf/client.go and oprf/server.go, on ristretto255_dev.h.
//
// A proof belongs to a REQUEST: a ragged group of 1 .. 65535 element pairs (B_j, kB_j).  Two launches per call:
//   composite<VERIFY>  one lane per ELEMENT.  The lane finds its request by an upper-bound search over the offsets (empty requests are
//                      skipped), recomputes the request's seed, hashes d_j and multiplies: d_j B_j, and d_j kB_j when verifying.  Then a
//                      segmented reduction inside the wavefront: six __shfl_down steps over the 40 words of a point and the request
//                      index; a lane adds what it received only if the sender exists and is of the same request.  Requests are
//                      contiguous, so the first lane of every request segment of the wave ends up with the segment's sum, and writes
//                      it to workspace slot (wave + request): unique and increasing along the (wave, request) pairs, at most
//                      ceil(n_elems / 64) + n_req slots.  Every lane reaches every shuffle: a lane beyond n_elems or with a failed
//                      element carries the neutral element, and a failed element raises the request's flag in the workspace.
//   finish<VERIFY>     one lane per REQUEST: adds the request's slots (contiguous, at most 1025) and runs the prover's or verifier's tail.
// d_j and the elements are public; the prover's k M, r M, r G and s = r - c k act on secrets and use the constant-time routines.  Nothing
// secret reaches the workspace.  The hashes are functions of their own (noinline), as in oprf_group_kernels.h.
//
// The POPRF items are of the shape of oprf_group_kernels.h (one item per lane, ristretto255 only) with an argument struct of their own: two ragged arguments.
#pragma once
#include <hip/hip_runtime.h>

#include "oprf_group_kernels.h"

namespace circl {
namespace dleq {

using ed25519::Ge;
using oprf::load8;
using oprf::store_masked;
using oprf::wipe;

constexpr int WAVES = oprf::WAVES;
constexpr uint64_t kMaxBatch = 0xffff;   // the index j travels as two bytes
constexpr uint32_t kNoIdentity = 1u;     // flags bit 0
constexpr int kTagHead = 13;             // "HashToScalar-"
constexpr int PW = 40;                   // words of a point in the workspace

struct Args {
    const uint64_t *off;       // n_req + 1 offsets, in elements << off_shift (the host pipeline's are bytes: shift 5)
    uint32_t off_shift;
    const uint32_t *B, *kB;    // rows of 8 words, indexed by the ABSOLUTE element index off[g] >> off_shift
    const uint32_t *k;         // prove: rows of 8 words, k_stride words apart (0: one key for the call)
    size_t k_stride;
    const uint32_t *kA;
    size_t kA_stride;
    const uint32_t *r;         // prove: rows of 8 words
    uint32_t *proofs;          // rows of 16 words, c || s: prove writes them, verify reads them
    uint8_t *ok;               // prove: may be nullptr
    uint32_t *partial;         // workspace: slots of PW (prove) or 2 PW (verify) words
    uint32_t *bad;             // workspace: one word per request, zero before composite runs
    size_t n_req, n_elems;
    uint32_t flags, tag_len;
    uint8_t tag[256];          // "HashToScalar-" || ctx; "Seed-" || ctx is made from its tail
};

CIRCL_HD uint64_t elem_off(const Args &a, size_t g) { return a.off[g] >> a.off_shift; }

// the request of absolute element e, off[0] <= e < off[n_req]: the LAST g with off[g] <= e, so that empty requests are skipped
CIRCL_HD size_t request_of(const Args &a, uint64_t e) {
    size_t lo = 0, hi = a.n_req;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (elem_off(a, mid) <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

CIRCL_HD void ge_store(uint32_t *w, const Ge &p) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        w[i] = p.X.v[i];
        w[10 + i] = p.Y.v[i];
        w[20 + i] = p.Z.v[i];
        w[30 + i] = p.T.v[i];
    }
}
CIRCL_HD Ge ge_load(const uint32_t *w) {
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
CIRCL_HD void put_row(uint8_t *m, const uint32_t *w, int words) {
    for (int i = 0; i < 4 * words; i++) m[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// seed = SHA-512(I2(32) || kA || I2(len("Seed-" || ctx)) || "Seed-" || ctx)
template <int WV>
CIRCL_HKDF_STREAM_CALL(WV) void seed_hash(uint32_t *seed, const uint32_t *kA, const uint8_t *tag, uint32_t tag_len) {
    hkdf::Stream<hkdf::Sha512, WV> st;
    const uint32_t ctx_len = tag_len - kTagHead, dst_len = 5 + ctx_len;
    st.init();
    st.put((uint8_t)0);
    st.put((uint8_t)32);
    st.put(reinterpret_cast<const uint8_t *>(kA), 32);
    st.put((uint8_t)(dst_len >> 8));
    st.put((uint8_t)dst_len);
    const char label[] = "Seed-";
    for (int j = 0; j < 5; j++) st.put((uint8_t)label[j]);
    st.put(tag + kTagHead, ctx_len);
    st.finish(seed);
}

// d_j = HashToScalar(I2(64) || seed || I2(j) || I2(32) || B_j || I2(32) || kB_j || "Composite", tag)
CIRCL_HD void composite_scalar(uint32_t d[8], const uint32_t seed[16], uint32_t j, const uint32_t b[8], const uint32_t kb[8], const uint8_t *tag,
                               uint32_t tag_len) {
    uint8_t m[145];
    uint32_t u[16];
    m[0] = 0; m[1] = 64;
    put_row(m + 2, seed, 16);
    m[66] = (uint8_t)(j >> 8); m[67] = (uint8_t)j;
    m[68] = 0; m[69] = 32;
    put_row(m + 70, b, 8);
    m[102] = 0; m[103] = 32;
    put_row(m + 104, kb, 8);
    const char label[] = "Composite";
    for (int i = 0; i < 9; i++) m[136 + i] = (uint8_t)label[i];
    hkdf::xmd<hkdf::Sha512, WAVES>(u, 64, m, 145, nullptr, 0, nullptr, 0, tag, tag_len);
    r255::sc_from_uniform(d, u);
}

// c = HashToScalar(I2(32) || kA || I2(32) || M || I2(32) || Z || I2(32) || t2 || I2(32) || t3 || "Challenge", tag); rows = the five encodings
CIRCL_HD void challenge_scalar(uint32_t c[8], const uint32_t rows[40], const uint8_t *tag, uint32_t tag_len) {
    uint8_t m[179];
    uint32_t u[16];
    for (int e = 0; e < 5; e++) {
        m[34 * e] = 0;
        m[34 * e + 1] = 32;
        put_row(m + 34 * e + 2, rows + 8 * e, 8);
    }
    const char label[] = "Challenge";
    for (int i = 0; i < 9; i++) m[170 + i] = (uint8_t)label[i];
    hkdf::xmd<hkdf::Sha512, WAVES>(u, 64, m, 179, nullptr, 0, nullptr, 0, tag, tag_len);
    r255::sc_from_uniform(c, u);
    for (int i = 0; i < 179; i++) m[i] = 0;   // (the prover's Z and t3 are derived from secrets)
    wipe<16>(u);
}

// The lane-local part of composite: m = d_j B_j and, when verifying, z = d_j kB_j for absolute element e of request g.  Returns 0
// (and neutral elements) where the request cannot be proven: more than 65535 pairs, kA or an element that does not decode, an identity
// element under kNoIdentity.  Everything here is public.
template <bool VERIFY>
CIRCL_HD uint32_t element(Ge &m, Ge &z, const Args &a, size_t g, uint64_t e) {
    const uint64_t first = elem_off(a, g), cnt = elem_off(a, g + 1) - first;
    uint32_t ka[8], b[8], kb[8], seed[16], d[8];
    load8(ka, a.kA + g * a.kA_stride);
    load8(b, a.B + 8 * e);
    load8(kb, a.kB + 8 * e);
    Ge pa, pb, pkb;
    uint32_t good = (cnt <= kMaxBatch ? 1u : 0u) & r255::r255_decode(pa, ka) & r255::r255_decode(pb, b) & r255::r255_decode(pkb, kb);
    if (a.flags & kNoIdentity) good &= (r255::r255_equal_identity(b) || r255::r255_equal_identity(kb)) ? 0u : 1u;
    m = ed25519::ge_identity();
    z = ed25519::ge_identity();
    if (!good) return 0;
    seed_hash<WAVES>(seed, ka, a.tag, a.tag_len);
    composite_scalar(d, seed, (uint32_t)(e - first), b, kb, a.tag, a.tag_len);
    m = r255::r255_mul(d, pb);
    if (VERIFY) z = r255::r255_mul(d, pkb);
    return 1;
}

CIRCL_HD void neg_mod_order(uint32_t out[8], const uint32_t c[8]) {  // L - c for c below L (c = 0 gives L, which the product reduces)
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)ed25519::order_word(i) - c[i] - borrow;
        out[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
}

// k P as a call: the tails multiply two to four times, and one copy of the loop keeps its registers (the pattern of the hashes)
template <int WV>
CIRCL_HKDF_STREAM_CALL(WV) void mul_call(Ge &out, const uint32_t *k, const Ge &p) {
    out = r255::r255_mul(k, p);
}

// The prover's tail for request g on its composite M: Z = k M, t2 = r G, t3 = r M, c, s = r - c k.  k and r are secrets.
CIRCL_HD void prove_tail(const Args &a, size_t g, const Ge &M, uint32_t good) {
    uint32_t k[8], r[8], rows[40], c[8], nc[8], proof[16];
    load8(k, a.k + g * a.k_stride);
    load8(r, a.r + 8 * g);
    load8(rows, a.kA + g * a.kA_stride);
    good &= oprf::secret_scalar_ok<oprf::R255>(k) & oprf::secret_scalar_ok<oprf::R255>(r);
    Ge p;
    mul_call<WAVES>(p, k, M);
    r255::r255_encode(rows + 8, M);
    r255::r255_encode(rows + 16, p);
    p = r255::r255_base(r);
    r255::r255_encode(rows + 24, p);
    mul_call<WAVES>(p, r, M);
    r255::r255_encode(rows + 32, p);
    challenge_scalar(c, rows, a.tag, a.tag_len);
    neg_mod_order(nc, c);
    ed25519::sc_muladd(proof + 8, nc, k, r);
#pragma unroll
    for (int i = 0; i < 8; i++) proof[i] = c[i];
    store_masked<16>(a.proofs + 16 * g, proof, good);
    if (a.ok) a.ok[g] = (uint8_t)good;
    wipe<8>(k);
    wipe<8>(r);
    wipe<40>(rows);
    wipe<16>(proof);
    wipe(p);
}

// The verifier's tail for request g on its composites M and Z: t2 = s G + c kA, t3 = s M + c Z; the verdict is "the recomputed c equals c"
CIRCL_HD void verify_tail(const Args &a, size_t g, const Ge &M, const Ge &Z, uint32_t good) {
    uint32_t proof[16], rows[40], c[8];
    for (int i = 0; i < 16; i++) proof[i] = a.proofs[16 * g + i];
    load8(rows, a.kA + g * a.kA_stride);
    Ge pa;
    good &= ed25519::sc_is_canonical(proof) & ed25519::sc_is_canonical(proof + 8) & r255::r255_decode(pa, rows);
    r255::r255_encode(rows + 8, M);
    r255::r255_encode(rows + 16, Z);
    Ge t, u;
    mul_call<WAVES>(u, proof, pa);
    t = r255::r255_add(r255::r255_base(proof + 8), u);
    r255::r255_encode(rows + 24, t);
    mul_call<WAVES>(t, proof + 8, M);
    mul_call<WAVES>(u, proof, Z);
    t = r255::r255_add(t, u);
    r255::r255_encode(rows + 32, t);
    challenge_scalar(c, rows, a.tag, a.tag_len);
    good &= ed25519::words_equal(c, proof) ? 1u : 0u;
    a.ok[g] = (uint8_t)good;
}

template <bool VERIFY>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void composite(const Args a) {
    const size_t lane_e = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = lane_e < a.n_elems;
    unsigned long long g = a.n_req;   // of no request: a lane beyond the elements never joins a live lane's sum
    Ge m = ed25519::ge_identity(), z = ed25519::ge_identity();
    if (live) {
        const uint64_t e = elem_off(a, 0) + lane_e;
        g = request_of(a, e);
        if (!element<VERIFY>(m, z, a, (size_t)g, e)) a.bad[g] = 1u;
    }
    // the segmented reduction: every lane of the wave takes every shuffle
    uint32_t mw[PW], zw[PW];
    ge_store(mw, m);
    if (VERIFY) ge_store(zw, z);
#pragma unroll 1
    for (unsigned d = 1; d < 64; d <<= 1) {
        const unsigned long long g2 = __shfl_down(g, d);
        uint32_t rw[PW];
#pragma unroll
        for (int i = 0; i < PW; i++) rw[i] = __shfl_down(mw[i], d);
        const bool take = threadIdx.x + d < 64 && g2 == g;
        if (take) ge_store(mw, r255::r255_add(ge_load(mw), ge_load(rw)));
        if (VERIFY) {
#pragma unroll
            for (int i = 0; i < PW; i++) rw[i] = __shfl_down(zw[i], d);
            if (take) ge_store(zw, r255::r255_add(ge_load(zw), ge_load(rw)));
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

template <bool VERIFY>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void finish(const Args a) {
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= a.n_req) return;
    const uint64_t first = elem_off(a, g) - elem_off(a, 0), cnt = elem_off(a, g + 1) - elem_off(a, g);
    const uint32_t good = (cnt >= 1 && cnt <= kMaxBatch && first + cnt <= a.n_elems && !a.bad[g]) ? 1u : 0u;   // (n_elems: the slots that exist)
    Ge M = ed25519::ge_identity(), Z = ed25519::ge_identity();
    if (good) {
        const size_t w1 = (size_t)((first + cnt - 1) / 64);
#pragma unroll 1
        for (size_t w = (size_t)(first / 64); w <= w1; w++) {
            const uint32_t *slot = a.partial + (w + g) * (VERIFY ? 2 * PW : PW);
            M = r255::r255_add(M, ge_load(slot));
            if (VERIFY) Z = r255::r255_add(Z, ge_load(slot + PW));
        }
    }
    if (VERIFY) verify_tail(a, g, M, Z, good);
    else prove_tail(a, g, M, good);
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
    const uint32_t *elems;     // pkS (tweak client; elem_stride words apart, 0: one key) or evaluated elements (finalize)
    size_t elem_stride;
    uint32_t *out, *out2, *out3;   // tweak server: t, t^-1, t G; tweak client: the tweaked key; finalize / full_evaluate: rows of 16 words
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

// "HashToScalar-" || "OPRFV1-" || 2 || "-ristretto255-SHA512" (41 bytes) or "HashToGroup-" || the same (40)
CIRCL_HD uint32_t mode2_tag(uint8_t *tag, bool to_group) {
    const char *head = to_group ? "HashToGroup-OPRFV1-" : "HashToScalar-OPRFV1-";
    uint32_t at = 0;
    for (const char *s = head; *s; s++) tag[at++] = (uint8_t)*s;
    tag[at++] = 2;
    for (const char *s = "-ristretto255-SHA512"; *s; s++) tag[at++] = (uint8_t)*s;
    return at;
}

// m = HashToScalar("Info" || I2(len) || info, "HashToScalar-" || ctx_2)
CIRCL_HD void info_scalar(uint32_t m[8], const uint8_t *info, uint64_t len) {
    uint8_t tag[48], pre[6] = {'I', 'n', 'f', 'o', (uint8_t)(len >> 8), (uint8_t)len};
    uint32_t u[16];
    const uint32_t tag_len = mode2_tag(tag, false);
    hkdf::xmd<hkdf::Sha512, WAVES>(u, 64, pre, 6, info, len, nullptr, 0, tag, tag_len);
    r255::sc_from_uniform(m, u);
}

// SHA-512(I2(len) || input || I2(len) || info || I2(32) || element || "Finalize")
template <int WV>
CIRCL_HKDF_STREAM_CALL(WV) void finalize_hash2(uint32_t *out, const uint8_t *input, uint64_t len, const uint8_t *info, uint64_t info_len, const uint32_t *element) {
    hkdf::Stream<hkdf::Sha512, WV> st;
    st.init();
    st.put((uint8_t)(len >> 8));
    st.put((uint8_t)len);
    st.put(input, len);
    st.put((uint8_t)(info_len >> 8));
    st.put((uint8_t)info_len);
    st.put(info, info_len);
    st.put((uint8_t)0);
    st.put((uint8_t)32);
    st.put(reinterpret_cast<const uint8_t *>(element), 32);
    const char tag[] = "Finalize";
    for (int j = 0; j < 8; j++) st.put((uint8_t)tag[j]);
    st.finish(out);
}

// t = sk + m, or zero words and verdict 0 where sk is no key, the info is too long or t = 0 (ErrInverseZero)
CIRCL_HD uint32_t tweaked_secret(uint32_t t[8], const ItemArgs &a, size_t i, const uint8_t *info, uint64_t info_len) {
    const bool fits = info_len <= oprf::kMaxInputBytes;
    uint32_t sk[8], m[8];
    const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    load8(sk, a.scalars + i * a.scalar_stride);
    info_scalar(m, info, fits ? info_len : 0);
    ed25519::sc_muladd(t, sk, one, m);
    const uint32_t good = oprf::secret_scalar_ok<oprf::R255>(sk) & (fits ? 1u : 0u) & (r255::sc_is_zero(t) ? 0u : 1u);
    wipe<8>(sk);
    return good;
}

template <int OP>
CIRCL_HD void item(const ItemArgs &a, size_t i);

template <>
CIRCL_HD void item<kTweakServer>(const ItemArgs &a, size_t i) {
    const uint8_t *info;
    const uint64_t info_len = rag(info, a.info, a.info_off, i);
    uint32_t t[8], tinv[8], enc[8];
    const uint32_t good = tweaked_secret(t, a, i, info, info_len);
    r255::sc_inv(tinv, t);
    Ge p = r255::r255_base(t);
    r255::r255_encode(enc, p);
    store_masked<8>(a.out + 8 * i, t, good);
    store_masked<8>(a.out2 + 8 * i, tinv, good);
    store_masked<8>(a.out3 + 8 * i, enc, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<8>(t);
    wipe<8>(tinv);
    wipe(p);
}

template <>
CIRCL_HD void item<kTweakClient>(const ItemArgs &a, size_t i) {
    const uint8_t *info;
    const uint64_t info_len = rag(info, a.info, a.info_off, i);
    const bool fits = info_len <= oprf::kMaxInputBytes;
    uint32_t pk[8], m[8], enc[8];
    load8(pk, a.elems + i * a.elem_stride);
    Ge p;
    uint32_t good = r255::r255_decode(p, pk) & (fits ? 1u : 0u);
    info_scalar(m, info, fits ? info_len : 0);
    p = r255::r255_add(r255::r255_base(m), p);
    r255::r255_encode(enc, p);
    good &= r255::r255_equal_identity(enc) ? 0u : 1u;
    store_masked<8>(a.out + 8 * i, enc, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
}

template <>
CIRCL_HD void item<kPoprfFinalize>(const ItemArgs &a, size_t i) {
    const uint8_t *m, *info;
    const uint64_t len = rag(m, a.input, a.input_off, i), info_len = rag(info, a.info, a.info_off, i);
    const bool fits = len <= oprf::kMaxInputBytes && info_len <= oprf::kMaxInputBytes;
    uint32_t k[8], kinv[8], e[8], enc[8], h[16];
    load8(k, a.scalars + i * a.scalar_stride);
    load8(e, a.elems + 8 * i);
    Ge p;
    const uint32_t good = oprf::secret_scalar_ok<oprf::R255>(k) & r255::r255_decode(p, e) & (r255::r255_equal_identity(e) ? 0u : 1u) & (fits ? 1u : 0u);
    r255::sc_inv(kinv, k);
    p = r255::r255_mul(kinv, p);
    r255::r255_encode(enc, p);
    finalize_hash2<WAVES>(h, m, fits ? len : 0, info, fits ? info_len : 0, enc);
    store_masked<16>(a.out + 16 * i, h, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<8>(k);
    wipe<8>(kinv);
    wipe<8>(enc);
    wipe<16>(h);
    wipe(p);
}

template <>
CIRCL_HD void item<kPoprfFullEvaluate>(const ItemArgs &a, size_t i) {
    const uint8_t *m, *info;
    const uint64_t len = rag(m, a.input, a.input_off, i), info_len = rag(info, a.info, a.info_off, i);
    const bool fits = len <= oprf::kMaxInputBytes;
    uint8_t tag[48];
    uint32_t u[16], t[8], tinv[8], enc[8], h[16];
    uint32_t good = tweaked_secret(t, a, i, info, info_len) & (fits ? 1u : 0u);
    r255::sc_inv(tinv, t);
    const uint32_t tag_len = mode2_tag(tag, true);
    hkdf::xmd<hkdf::Sha512, WAVES>(u, 64, nullptr, 0, m, fits ? len : 0, nullptr, 0, tag, tag_len);
    Ge p = r255::r255_from_uniform(u);
    p = r255::r255_mul(tinv, p);
    r255::r255_encode(enc, p);
    good &= r255::r255_equal_identity(enc) ? 0u : 1u;
    finalize_hash2<WAVES>(h, m, fits ? len : 0, info, info_len <= oprf::kMaxInputBytes ? info_len : 0, enc);
    store_masked<16>(a.out + 16 * i, h, good);
    if (a.ok) a.ok[i] = (uint8_t)good;
    wipe<16>(u);
    wipe<8>(t);
    wipe<8>(tinv);
    wipe<8>(enc);
    wipe<16>(h);
    wipe(p);
}

template <int OP>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void item_kernel(const ItemArgs a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    item<OP>(a, i);
}

}  // namespace dleq
}  // namespace circl
