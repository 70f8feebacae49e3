// nistp_kernels.h -- batch P-256 / P-384 group operations (group/short.go) and the proof-free part of OPRF (RFC 9497, suites P256-SHA256
// and P384-SHA384; oprf/keys.go, oprf/client.go, oprf/server.go) on nistp_dev.h: one item per lane, one launch per call, no workspace.
//
// The pattern of oprf_kernels.h: one item function per public operation and curve (item<C, OP, WV>), one kernel per item function.
// expand_message_xmd and the Finalize hash are functions of their own (nistp::xmd, finalize_hash), so that the field loops of the
// multiplication keep their register allocation and what a hash holds does not live across them.  A hashed point, an evaluated element
// before it is hashed, a blind's inverse: none of them reaches memory.
//
// Failure is a mask: ok[i] = 0 and every output row of item i is zero.  The verdicts are computed without a branch on a secret; only
// lengths (public) steer loops.  Secrets a lane held are zeroed before it returns.
//
// Rows: scalars, keys and blinds are NS = 32 / 48 big-endian bytes, read as words (4-byte aligned); seeds are 32 bytes and OPRF outputs
// NH = 32 / 48 bytes, words too; elements are packed rows of NE = 33 / 49 bytes, read and written bytewise (no alignment).
//
// What the compiler reports for gfx950 (-Rpass-analysis=kernel-resource-usage; WAVES = 2 allows 256 registers), VGPRs / scratch bytes
// per lane, occupancy 2 waves per SIMD for every kernel:
//                     P-256        P-384                             P-256        P-384
//   hash_to_group     180 / 640    256 / 944       blind             233 / 640    256 / 2496
//   hash_to_scalar    180 / 608    248 / 800       evaluate          243 / 0      256 / 1472
//   scalar_mult       208 / 0      256 / 208       finalize          244 / 224    256 / 1824
//   derive_keypair    197 / 672    256 / 912       full_evaluate     237 / 720    256 / 2624
// P-256's field loops use no scratch (what the hashing kernels report is the hash streams' buffers, passed by address).  P-384's
// twelve-limb points do NOT fit 256 registers: the bare multiplication spills 208 bytes (52 words) per lane, the kernels that also
// decode or hash more.  Correctness and constant time were not traded for registers.
#pragma once
#include <hip/hip_runtime.h>

#include "nistp_dev.h"

namespace circl {
namespace nistp {

constexpr int WAVES = 2;  // the Ed25519 kernels' class: two points and a product's temporaries in 256 registers
constexpr uint64_t kMaxInputBytes = 0xffff;  // RFC 9497: inputs and infos carry a two-byte length

enum Op : int { kHashToGroup = 0, kHashToScalar, kScalarMult, kDeriveKeyPair, kBlind, kEvaluate, kFinalize, kFullEvaluate, kOps };

struct Args {
    const uint8_t *blob;       // the ragged argument (messages, infos, inputs); nullptr: every item's is empty
    const uint64_t *off;
    const uint32_t *scalars;   // rows of N words, scalar_stride words apart (0: one row for the batch): scalars, keys, blinds
    size_t scalar_stride;
    const uint8_t *elems;      // rows of NE bytes: elements, blinded / evaluated elements; nullptr (kScalarMult): the generator
    const uint32_t *seeds;     // kDeriveKeyPair: rows of 8 words
    uint8_t *out;              // rows of NE bytes (elements), or of N words (kHashToScalar, kDeriveKeyPair: sk), or of NH / 4 words (outputs)
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
template <int N>
CIRCL_HD void wipe(Fe<N> &x) { wipe<N>(x.v); }
template <class C>
CIRCL_HD void wipe(Pt<C> &p) {
    wipe(p.X);
    wipe(p.Y);
    wipe(p.Z);
}
// 1 for a scalar a key or a blind may be: canonical and not zero
template <class C>
CIRCL_HD uint32_t secret_scalar_ok(const Fe<C::N> &k) { return sc_is_canonical<C>(k) & (sc_is_zero<C>(k) ? 0u : 1u); }

// oprf/client.go Finalize / server.go FullEvaluate: H(I2OSP(len, 2) || input || I2OSP(NE, 2) || element || "Finalize")
template <class C, int WV>
CIRCL_HKDF_STREAM_CALL(WV) void finalize_hash(uint32_t *out, const uint8_t *input, uint64_t len, const uint32_t *element) {
    hkdf::Stream<typename C::Hash, WV> st;
    st.init();
    st.put((uint8_t)(len >> 8));
    st.put((uint8_t)len);
    st.put(input, len);
    st.put((uint8_t)0);
    st.put((uint8_t)C::NE);
    st.put(reinterpret_cast<const uint8_t *>(element), C::NE);
    const char tag[] = "Finalize";
    for (int j = 0; j < 8; j++) st.put((uint8_t)tag[j]);
    st.finish(out);
}

template <class C, int OP, int WV>
struct Item;

// group.P256 / P384 HashToElement(msg, dst), or HashToElementNonUniform where flags & 1
template <class C, int WV>
struct Item<C, kHashToGroup, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool nu = (a.flags & 1u) != 0;  // (a launch-wide flag)
        uint32_t u[uniform_words<C, 2>()], enc[elem_words<C>()];
        xmd<typename C::Hash, WV>(u, nu ? C::L : 2 * C::L, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
        nistp_encode<C>(enc, nistp_from_uniform<C>(u, nu));
        elem_store<C>(a.out + (size_t)C::NE * i, enc, 1);
    }
};

// group.P256 / P384 HashToScalar(msg, dst)
template <class C, int WV>
struct Item<C, kHashToScalar, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        uint32_t u[uniform_words<C, 1>()];
        xmd<typename C::Hash, WV>(u, C::L, nullptr, 0, m, len, nullptr, 0, a.dst, a.dst_len);
        sc_store<C>(reinterpret_cast<uint32_t *>(a.out) + C::N * i, sc_from_uniform<C>(u), 1);
    }
};

// Element.Mul / Element.MulGen, optionally by the scalar's inverse: the scalar below n, the element any valid one (the identity too)
template <class C, int WV>
struct Item<C, kScalarMult, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        uint32_t enc[elem_words<C>()];
        Fe<C::N> k = sc_load<C>(a.scalars + i * a.scalar_stride);
        uint32_t good = sc_is_canonical<C>(k);
        if (a.flags & 1u) {  // (a launch-wide flag)
            good &= sc_is_zero<C>(k) ? 0u : 1u;
            k = sc_inv<C>(k);
        }
        Pt<C> p = pt_generator<C>();
        if (a.elems) {
            elem_load<C>(enc, a.elems + (size_t)C::NE * i);
            good &= nistp_decode<C>(p, enc);
        }
        p = nistp_mul<C>(k, p);
        nistp_encode<C>(enc, p);
        elem_store<C>(a.out + (size_t)C::NE * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe(k);
        wipe(p);
    }
};

// oprf/keys.go DeriveKey: sk = HashToScalar(seed || I2OSP(len(info), 2) || info || counter, "DeriveKeyPair" || ctx) for the first
// counter in 0..255 that gives a non-zero scalar, pk = sk G.  The loop ends on "the scalar is not zero": a scalar that the loop
// discards is never a key, and that a candidate was zero says nothing about the one that is kept.
template <class C, int WV>
struct Item<C, kDeriveKeyPair, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *info;
        const uint64_t info_len = item_range(info, a, i);
        const bool fits = info_len <= kMaxInputBytes;
        uint32_t pre[9], u[uniform_words<C, 1>()], pk[elem_words<C>()];
#pragma unroll
        for (int j = 0; j < 8; j++) pre[j] = a.seeds[8 * i + j];
        pre[8] = (uint32_t)((info_len >> 8) & 0xff) | (uint32_t)(info_len & 0xff) << 8;
        uint32_t good = 0;
        Fe<C::N> sk = fe_zero<typename C::Fn>();
        for (uint32_t counter = 0; counter < 256 && !good; counter++) {
            const uint8_t c = (uint8_t)counter;
            xmd<typename C::Hash, WV>(u, C::L, reinterpret_cast<const uint8_t *>(pre), 34, info, fits ? info_len : 0, &c, 1, a.dst, a.dst_len);
            sk = sc_from_uniform<C>(u);
            good = sc_is_zero<C>(sk) ? 0u : 1u;
        }
        good &= fits ? 1u : 0u;
        Pt<C> p = nistp_base<C>(sk);
        nistp_encode<C>(pk, p);
        sc_store<C>(reinterpret_cast<uint32_t *>(a.out) + C::N * i, sk, good);
        elem_store<C>(a.out2 + (size_t)C::NE * i, pk, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<9>(pre);
        wipe<uniform_words<C, 1>()>(u);
        wipe(sk);
        wipe(p);
    }
};

// oprf/client.go DeterministicBlind: blinded = blind HashToGroup(input)
template <class C, int WV>
struct Item<C, kBlind, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t u[uniform_words<C, 2>()], enc[elem_words<C>()];
        Fe<C::N> k = sc_load<C>(a.scalars + i * a.scalar_stride);
        uint32_t good = secret_scalar_ok<C>(k) & (fits ? 1u : 0u);
        xmd<typename C::Hash, WV>(u, 2 * C::L, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
        Pt<C> p = nistp_from_uniform<C>(u, false);
        p = nistp_mul<C>(k, p);
        // blind != 0 and the group has prime order: the blinded element is the identity exactly where the hashed point is
        good &= nistp_encode<C>(enc, p) ^ 1u;
        elem_store<C>(a.out + (size_t)C::NE * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<uniform_words<C, 2>()>(u);
        wipe(k);
        wipe(p);
    }
};

// oprf/server.go Server.Evaluate (base mode): evaluated = sk blinded
template <class C, int WV>
struct Item<C, kEvaluate, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        uint32_t enc[elem_words<C>()], ident;
        Fe<C::N> k = sc_load<C>(a.scalars + i * a.scalar_stride);
        elem_load<C>(enc, a.elems + (size_t)C::NE * i);
        Pt<C> p;
        uint32_t good = secret_scalar_ok<C>(k) & nistp_decode<C>(p, enc, &ident);
        good &= ident ^ 1u;
        p = nistp_mul<C>(k, p);
        nistp_encode<C>(enc, p);
        elem_store<C>(a.out + (size_t)C::NE * i, enc, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe(k);
        wipe(p);
    }
};

// oprf/client.go Client.Finalize (base mode): output = Hash(input, blind^-1 evaluated)
template <class C, int WV>
struct Item<C, kFinalize, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        constexpr int HW = C::Hash::OUT / 4;
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t enc[elem_words<C>()], h[HW], ident;
        Fe<C::N> k = sc_load<C>(a.scalars + i * a.scalar_stride);
        elem_load<C>(enc, a.elems + (size_t)C::NE * i);
        Pt<C> p;
        uint32_t good = secret_scalar_ok<C>(k) & nistp_decode<C>(p, enc, &ident) & (fits ? 1u : 0u);
        good &= ident ^ 1u;
        Fe<C::N> kinv = sc_inv<C>(k);
        p = nistp_mul<C>(kinv, p);
        nistp_encode<C>(enc, p);
        finalize_hash<C, WV>(h, m, fits ? len : 0, enc);
        store_masked<HW>(reinterpret_cast<uint32_t *>(a.out) + HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe(k);
        wipe(kinv);
        wipe<elem_words<C>()>(enc);
        wipe<HW>(h);
        wipe(p);
    }
};

// oprf/server.go Server.FullEvaluate / VerifiableServer.FullEvaluate: output = Hash(input, sk HashToGroup(input))
template <class C, int WV>
struct Item<C, kFullEvaluate, WV> {
    static CIRCL_HD void run(const Args &a, size_t i) {
        constexpr int HW = C::Hash::OUT / 4;
        const uint8_t *m;
        const uint64_t len = item_range(m, a, i);
        const bool fits = len <= kMaxInputBytes;
        uint32_t u[uniform_words<C, 2>()], enc[elem_words<C>()], h[HW];
        Fe<C::N> k = sc_load<C>(a.scalars + i * a.scalar_stride);
        uint32_t good = secret_scalar_ok<C>(k) & (fits ? 1u : 0u);
        xmd<typename C::Hash, WV>(u, 2 * C::L, nullptr, 0, m, fits ? len : 0, nullptr, 0, a.dst, a.dst_len);
        Pt<C> p = nistp_from_uniform<C>(u, false);
        p = nistp_mul<C>(k, p);
        good &= nistp_encode<C>(enc, p) ^ 1u;  // as in kBlind: the hashed point was the identity
        finalize_hash<C, WV>(h, m, fits ? len : 0, enc);
        store_masked<HW>(reinterpret_cast<uint32_t *>(a.out) + HW * i, h, good);
        if (a.ok) a.ok[i] = (uint8_t)good;
        wipe<uniform_words<C, 2>()>(u);
        wipe(k);
        wipe<elem_words<C>()>(enc);
        wipe<HW>(h);
        wipe(p);
    }
};

template <class C, int OP>
static __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    Item<C, OP, WAVES>::run(a, i);
}

}  // namespace nistp
}  // namespace circl
