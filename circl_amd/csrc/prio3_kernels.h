// prio3_kernels.h -- batch Prio3Count and Prio3Sum (draft-irtf-cfrg-vdaf-13 section 7; the reference's vdaf/prio3): Shard, PrepInit,
// PrepSharesToPrep and AggregateUpdate, one report per lane, over fp64_dev.h and prio3_xof_dev.h.
//
// The FLP (internal/flp/flp.go) is one template over a circuit, which names its gadget; Count (gadget Mul, arity 2, one call) and Sum
// (gadget x^2 - x, arity 1, 2 b calls) instantiate it.  Two things differ from the reference's order of work, both exact in the field:
//   * query() evaluates the gadget polynomial at alpha^1 .. alpha^calls by folding its 2P - 1 coefficients to P (c[j] + c[j + P]:
//     alpha^P = 1) and ONE size-P transform, not by `calls` Horner evaluations of length 2P - 1;
//   * a proof share is never held: its elements are folded, and accumulated into the evaluation at t with a running power of t, as they
//     leave the sampler (a helper) or the row (the leader).
// prove() gets the gadget polynomial from the wire polynomials' values at the 2P-th roots (a size-P inverse transform and a size-2P
// transform per wire, the gadget pointwise, one size-2P inverse transform), which is the reference's product of polynomials.
//
// What a lane keeps -- the wires, the folded polynomial, the query randomness: (2 arity P + MEAS_LEN + 1) elements, 3 KB at P = 128 --
// lives in a lane-interleaved global workspace (element j of item i at j * n_pad + i: every access of a wavefront is one contiguous
// 512 bytes), the sponge's block buffer in LDS (10.5 KB per wavefront).  All loop bounds and indices are public (the type, the batch's
// shares, lengths); nothing branches on or indexes by a secret.  The sampler's rejection (2^-32 per word) and the verdicts are the
// reference's own data-dependent exits.  A lane whose report fails runs on to the end and zeroes its rows there.
#pragma once
#include <hip/hip_runtime.h>

#include "prio3_xof_dev.h"

namespace circl {
namespace prio3 {

constexpr int COUNT = 1, SUM = 2;
constexpr int AGG_BLOCKS = 1024, AGG_THREADS = 256;   // the reduction's first launch: at most AGG_BLOCKS partial sums

// a task as the kernels see it: all public
struct Task {
    uint32_t kind, shares, bits, meas_len, calls, logp, p, arity;
    uint64_t max, offset;
    uint64_t range_const;   // Sum: offset * shares^-1
    uint64_t inv_p;         // P^-1
    Header hdr;
    CIRCL_HD uint32_t proof_len() const { return arity + 2 * p - 1; }
    CIRCL_HD uint32_t verifier_len() const { return 2 + arity; }
    CIRCL_HD uint32_t eval_out() const { return kind == COUNT ? 1 : meas_len + 1; }
    CIRCL_HD uint32_t query_rand_len() const { return 1 + eval_out(); }
    CIRCL_HD uint32_t leader_words() const { return meas_len + proof_len(); }
    CIRCL_HD uint32_t ws_elems() const { return 2 * arity * p + meas_len + 1; }
};

static inline bool task_ok(int kind, uint64_t max_measurement) {
    return kind == COUNT ? max_measurement == 0 : kind == SUM && max_measurement >= 1 && max_measurement < (uint64_t(1) << 63);
}
// kind / max_measurement checked by task_ok; shares in 2 .. 255
static inline Task make_task(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len) {
    Task t = {};
    t.kind = (uint32_t)kind;
    t.shares = (uint32_t)shares;
    t.max = max_measurement;
    if (kind == COUNT) {
        t.meas_len = t.calls = 1;
        t.arity = 2;
    } else {
        while (t.bits < 64 && (max_measurement >> t.bits)) t.bits++;
        t.meas_len = t.calls = 2 * t.bits;
        t.arity = 1;
        t.offset = (uint64_t(1) << t.bits) - 1 - max_measurement;
        t.range_const = fp64::mul(t.offset, fp64::inv((uint64_t)shares));
    }
    while ((1u << t.logp) < 1 + t.calls) t.logp++;
    t.p = 1u << t.logp;
    t.inv_p = fp64::inv_two_pow((int)t.logp);
    t.hdr = make_header((uint32_t)kind, ctx, ctx_len);
    return t;
}

// ---- transforms over a lane's array ------------------------------------------------------------------------------------------------
// v[k] <- sum_j v[j] w^(jk), w the root of order n = 2^lg (arith/fp64/vector.go NTT)
CIRCL_HD void ntt(Strided v, uint32_t lg) {
    const uint32_t n = 1u << lg;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t j = __builtin_bitreverse32(i) >> (32 - lg);
        if (i < j) {
            const uint64_t a = v[i], b = v[j];
            v[i] = b;
            v[j] = a;
        }
    }
    for (uint32_t l = 1; l <= lg; l++) {
        const uint32_t half = 1u << (l - 1);
        const uint64_t wn = fp64::root_of_unity((int)l);
        uint64_t w = 1;
        for (uint32_t i = 0; i < half; i++) {
            for (uint32_t s = i; s < n; s += 2 * half) {
                const uint64_t u = v[s], x = fp64::mul(w, v[s + half]);
                v[s] = fp64::add(u, x);
                v[s + half] = fp64::sub(u, x);
            }
            w = fp64::mul(w, wn);
        }
    }
}
// the coefficients of the polynomial with values v at w^0 .. w^(n-1), times `scale` (n^-1 for the coefficients themselves)
CIRCL_HD void intt(Strided v, uint32_t lg, uint64_t scale) {
    const uint32_t n = 1u << lg;
    ntt(v, lg);
    for (uint32_t i = 1; i < n - i; i++) {
        const uint64_t a = v[i], b = v[n - i];
        v[i] = b;
        v[n - i] = a;
    }
    if (scale != 1)
        for (uint32_t i = 0; i < n; i++) v[i] = fp64::mul(v[i], scale);
}
CIRCL_HD uint64_t horner(Strided c, uint32_t n, uint64_t x) {
    uint64_t r = c[n - 1];
    for (uint32_t i = n - 1; i-- > 0;) r = fp64::add(fp64::mul(r, x), c[i]);
    return r;
}

// ---- gadgets and circuits (internal/flp/gadgets.go, count/count.go, sum/sum.go) --------------------------------------------------------
struct GadgetMul {
    static constexpr uint32_t ARITY = 2;
    static CIRCL_HD uint64_t eval(const uint64_t *x) { return fp64::mul(x[0], x[1]); }
};
struct GadgetPolyEvalX2X {
    static constexpr uint32_t ARITY = 1;
    static CIRCL_HD uint64_t eval(const uint64_t *x) { return fp64::sub(fp64::sqr(x[0]), x[0]); }
};

// What query() accumulates while the measurement share goes by: the out share (Truncate) and the circuit's own linear part.
struct MeasAcc {
    uint64_t out = 0, lin = 0, pw = 1;
};

struct CircuitCount {
    using Gadget = GadgetMul;
    static constexpr int KIND = COUNT;
    static CIRCL_HD bool in_range(const Task &, uint64_t m) { return m <= 1; }
    // element j of the encoded measurement
    static CIRCL_HD uint64_t encode(const Task &, uint64_t m, uint32_t) { return m & 1; }
    static CIRCL_HD void on_meas(const Task &, MeasAcc &a, uint32_t, uint64_t e) { a.out = a.lin = e; }
    // the verifier's first element from the gadget's outputs g[1 .. calls] (g = the folded, transformed polynomial) and the randomness
    static CIRCL_HD uint64_t verdict(const Task &, const MeasAcc &a, Strided g, Strided) { return fp64::sub(g[1], a.lin); }
    static CIRCL_HD uint32_t t_index(const Task &) { return 0; }
};

struct CircuitSum {
    using Gadget = GadgetPolyEvalX2X;
    static constexpr int KIND = SUM;
    static CIRCL_HD bool in_range(const Task &t, uint64_t m) { return m <= t.max; }
    static CIRCL_HD uint64_t encode(const Task &t, uint64_t m, uint32_t j) { return j < t.bits ? (m >> j) & 1 : ((m + t.offset) >> (j - t.bits)) & 1; }
    // lin = sum 2^i meas[i] - sum 2^i meas[b + i]; out = the first sum
    static CIRCL_HD void on_meas(const Task &t, MeasAcc &a, uint32_t j, uint64_t e) {
        if (j == t.bits) {
            a.out = a.lin;
            a.pw = 1;
        }
        const uint64_t x = fp64::mul(e, a.pw);
        a.lin = j < t.bits ? fp64::add(a.lin, x) : fp64::sub(a.lin, x);
        a.pw = fp64::add(a.pw, a.pw);
    }
    static CIRCL_HD uint64_t verdict(const Task &t, const MeasAcc &a, Strided g, Strided r) {
        uint64_t v = fp64::mul(fp64::add(t.range_const, a.lin), r[t.meas_len]);
        for (uint32_t i = 0; i < t.meas_len; i++) v = fp64::add(v, fp64::mul(g[i + 1], r[i]));
        return v;
    }
    static CIRCL_HD uint32_t t_index(const Task &t) { return t.meas_len + 1; }
};

// ---- the FLP -----------------------------------------------------------------------------------------------------------------------
template <class C> struct Flp {
    using G = typename C::Gadget;
    static constexpr uint32_t A = G::ARITY;

    // Prove: ws[a * 2P + k], k < P, holds wire a's value at call k (k = 0: its seed) and zeros behind the calls; afterwards
    // ws[0 .. 2P - 1) is the gadget polynomial (ws[2P - 1] = 0: its degree is 2P - 2)
    static CIRCL_HD void prove(const Task &t, Strided ws) {
        const uint32_t p2 = 2 * t.p;
        for (uint32_t a = 0; a < A; a++) {
            Strided w = ws.from(a * p2);
            intt(w, t.logp, t.inv_p);
            for (uint32_t k = t.p; k < p2; k++) w[k] = 0;
            ntt(w, t.logp + 1);
        }
        for (uint32_t k = 0; k < p2; k++) {
            uint64_t x[A];
#pragma unroll
            for (uint32_t a = 0; a < A; a++) x[a] = ws[a * p2 + k];
            ws[k] = G::eval(x);
        }
        intt(ws, t.logp + 1, fp64::mul(t.inv_p, fp64::inv_two_pow(1)));
    }

    // Query, on a source that yields the query randomness (rand_begin, rand_next), then the measurement share (meas_begin, next) and
    // then the proof share (proof_begin, next).  ws: F[P] | wires[A][P] | R[eval_out].  verifier[2 + A]; false: ErrInvalidEval or a
    // source that failed.
    template <class Src> static CIRCL_HD bool query(const Task &t, Strided ws, Src &src, uint64_t *verifier, uint64_t &out_share) {
        Strided F = ws, W = ws.from(t.p), R = ws.from(t.p + A * t.p);
        bool ok = true;
        // the query randomness: eval_out coefficients for the circuit's outputs (none when there is one output), and t
        uint64_t tt = 0;
        const uint32_t ti = C::t_index(t);
        src.rand_begin();
        for (uint32_t i = 0; i < t.query_rand_len(); i++) {
            uint64_t e;
            ok &= src.rand_next(e);
            if (i == ti) tt = e;
            else if (i < ti) R[i] = e;
        }
        uint64_t tp = tt;
        for (uint32_t i = 0; i < t.logp; i++) tp = fp64::sqr(tp);
        ok &= tp != 1;
        // the measurement share: the wires' values at calls 1 .. calls
        MeasAcc acc;
        src.meas_begin();
        for (uint32_t j = 0; j < t.meas_len; j++) {
            uint64_t e;
            ok &= src.next(e);
            C::on_meas(t, acc, j, e);
            for (uint32_t a = 0; a < A; a++) W[a * t.p + 1 + j] = e;
        }
        out_share = acc.out;
        for (uint32_t a = 0; a < A; a++)
            for (uint32_t k = 1 + t.calls; k < t.p; k++) W[a * t.p + k] = 0;
        // the proof share: the wires' seeds, then the gadget polynomial -- folded, and evaluated at t, as it goes by
        src.proof_begin();
        for (uint32_t a = 0; a < A; a++) {
            uint64_t e;
            ok &= src.next(e);
            W[a * t.p] = e;
        }
        uint64_t gcheck = 0, tpow = 1;
        for (uint32_t j = 0; j < 2 * t.p - 1; j++) {
            uint64_t e;
            ok &= src.next(e);
            F[j & (t.p - 1)] = j < t.p ? e : fp64::add(F[j - t.p], e);
            gcheck = fp64::add(gcheck, fp64::mul(e, tpow));
            tpow = fp64::mul(tpow, tt);
        }
        ntt(F, t.logp);
        verifier[0] = C::verdict(t, acc, F, R);
        for (uint32_t a = 0; a < A; a++) {
            Strided w = W.from(a * t.p);
            intt(w, t.logp, 1);
            verifier[1 + a] = fp64::mul(horner(w, t.p, tt), t.inv_p);
        }
        verifier[1 + A] = gcheck;
        return ok;
    }

    static CIRCL_HD bool decide(const uint64_t *verifier) { return (verifier[0] == 0) & (G::eval(verifier + 1) == verifier[1 + A]); }
};

// ---- the operations, one report each ------------------------------------------------------------------------------------------------------
// What PrepInit draws its elements from.  One sponge serves every stream of a report: a stream is drained before the next begins.
struct QuerySrc {
    Xof x;
    const Task &t;
    const uint8_t *verify_key, *nonce;
    CIRCL_HD QuerySrc(Strided blk, const Task &t, const uint8_t *verify_key, const uint8_t *nonce) : x(blk), t(t), verify_key(verify_key), nonce(nonce) {}
    CIRCL_HD void rand_begin() { x.init(Msg{&t.hdr, QUERY_RAND, verify_key, 1, 1, 0, nonce}); }
    CIRCL_HD bool rand_next(uint64_t &e) { return sample(x, e); }
};
// a helper's shares: two streams under its seed
struct HelperSrc : QuerySrc {
    const uint8_t *seed;
    uint8_t agg_id;
    CIRCL_HD HelperSrc(Strided blk, const Task &t, const uint8_t *verify_key, const uint8_t *nonce, const uint8_t *seed, uint8_t agg_id)
        : QuerySrc(blk, t, verify_key, nonce), seed(seed), agg_id(agg_id) {}
    CIRCL_HD void meas_begin() { x.init(Msg{&t.hdr, MEAS_SHARE, seed, 1, agg_id, 0, nullptr}); }
    CIRCL_HD void proof_begin() { x.init(Msg{&t.hdr, PROOF_SHARE, seed, 2, 1, agg_id, nullptr}); }
    CIRCL_HD bool next(uint64_t &e) { return sample(x, e); }
};
// the leader's share: a row of elements, each of which must be canonical (the reference's Unmarshal)
struct LeaderSrc : QuerySrc {
    const uint64_t *row;
    CIRCL_HD LeaderSrc(Strided blk, const Task &t, const uint8_t *verify_key, const uint8_t *nonce, const uint64_t *row)
        : QuerySrc(blk, t, verify_key, nonce), row(row) {}
    CIRCL_HD void meas_begin() {}
    CIRCL_HD void proof_begin() {}
    CIRCL_HD bool next(uint64_t &e) {
        const uint64_t v = *row++;
        const bool ok = fp64::canonical(v);
        e = v & fp64::mask(ok);
        return ok;
    }
};

// Shard: leader[leader_words] (zeros and false for a measurement out of range or an exhausted sampler).  rand: the helpers' seeds,
// then the prove seed.  ws: ws_elems(), blk: RATE_WORDS.
template <class C> CIRCL_HD bool shard_item(const Task &t, uint64_t m, const uint8_t *rand, uint64_t *leader, Strided ws, Strided blk) {
    constexpr uint32_t A = Flp<C>::A;
    const uint32_t p2 = 2 * t.p;
    Strided M = ws.from(A * p2);
    bool ok = C::in_range(t, m);
    m &= fp64::mask(ok);
    uint64_t seeds[A], e;
    Xof x(blk);
    x.init(Msg{&t.hdr, PROVE_RAND, rand + SEED * (t.shares - 1), 1, 1, 0, nullptr});
#pragma unroll
    for (uint32_t a = 0; a < A; a++) {
        ok &= sample(x, seeds[a]);
        ws[a * p2] = seeds[a];
    }
    for (uint32_t j = 0; j < t.meas_len; j++) {
        e = C::encode(t, m, j);
        M[j] = e;
        for (uint32_t a = 0; a < A; a++) ws[a * p2 + 1 + j] = e;
    }
    for (uint32_t a = 0; a < A; a++)
        for (uint32_t k = 1 + t.calls; k < t.p; k++) ws[a * p2 + k] = 0;
    Flp<C>::prove(t, ws);
    // the leader's shares: what is left when the helpers' are taken off
    for (uint32_t j = 1; j < t.shares; j++) {
        const uint8_t *seed = rand + SEED * (j - 1);
        x.init(Msg{&t.hdr, MEAS_SHARE, seed, 1, (uint8_t)j, 0, nullptr});
        for (uint32_t i = 0; i < t.meas_len; i++) {
            ok &= sample(x, e);
            M[i] = fp64::sub(M[i], e);
        }
        x.init(Msg{&t.hdr, PROOF_SHARE, seed, 2, 1, (uint8_t)j, nullptr});
#pragma unroll
        for (uint32_t a = 0; a < A; a++) {
            ok &= sample(x, e);
            seeds[a] = fp64::sub(seeds[a], e);
        }
        for (uint32_t i = 0; i < p2 - 1; i++) {
            ok &= sample(x, e);
            ws[i] = fp64::sub(ws[i], e);
        }
    }
    const uint64_t keep = fp64::mask(ok);
    for (uint32_t i = 0; i < t.meas_len; i++) *leader++ = M[i] & keep;
#pragma unroll
    for (uint32_t a = 0; a < A; a++) *leader++ = seeds[a] & keep;
    for (uint32_t i = 0; i < p2 - 1; i++) *leader++ = ws[i] & keep;
    return ok;
}

// PrepInit: prep_share[verifier_len], out_share; zeros and false for a leader share that is not canonical, t^P = 1 or an exhausted
// sampler.  share: the leader share (agg_id 0) or a helper's seed.
template <class C> CIRCL_HD bool prep_init_item(const Task &t, uint32_t agg_id, const uint8_t *verify_key, const uint8_t *nonce, const void *share,
                                               uint64_t *prep_share, uint64_t *out_share, Strided ws, Strided blk) {
    constexpr uint32_t A = Flp<C>::A;
    uint64_t verifier[2 + A], out = 0;
    bool ok;
    if (agg_id == 0) {
        LeaderSrc src(blk, t, verify_key, nonce, static_cast<const uint64_t *>(share));
        ok = Flp<C>::query(t, ws, src, verifier, out);
    } else {
        HelperSrc src(blk, t, verify_key, nonce, static_cast<const uint8_t *>(share), (uint8_t)agg_id);
        ok = Flp<C>::query(t, ws, src, verifier, out);
    }
    const uint64_t keep = fp64::mask(ok);
#pragma unroll
    for (uint32_t k = 0; k < 2 + A; k++) prep_share[k] = verifier[k] & keep;
    *out_share = out & keep;
    return ok;
}

// PrepSharesToPrep: Decide on the sum of the aggregators' verifier shares; false too where an element is not canonical
template <class C> CIRCL_HD bool prep_finish_item(const Task &t, const uint64_t *prep_shares) {
    constexpr uint32_t V = 2 + Flp<C>::A;
    uint64_t verifier[V] = {};
    bool ok = true;
    for (uint32_t j = 0; j < t.shares; j++)
#pragma unroll
        for (uint32_t k = 0; k < V; k++) {
            const uint64_t e = prep_shares[j * V + k];
            ok &= fp64::canonical(e);
            verifier[k] = fp64::add(verifier[k], fp64::canon(e));
        }
    return ok & Flp<C>::decide(verifier);
}

// ---- kernels: one report per lane ------------------------------------------------------------------------------------------------------
struct Args {
    Task t;
    uint32_t agg_id;
    const uint64_t *measurement;   // shard
    const uint8_t *rand;           // shard: rows of 32 shares
    const uint8_t *verify_key;     // prep_init: one for the call
    const uint8_t *nonce;          // prep_init: rows of 16
    const uint8_t *share;          // prep_init: rows of leader_words() words (agg_id 0) or of 32 bytes; prep_finish: rows of shares * verifier_len() words
    uint64_t *leader;              // shard
    uint64_t *prep_share, *out_share;
    uint8_t *ok;                   // shard, prep_init: may be nullptr
    uint64_t *ws;                  // ws_elems() x n_pad words
    size_t n, n_pad;
};

#if defined(__HIPCC__)
#define PRIO3_LANE                                                        \
    __shared__ uint64_t blk_[RATE_WORDS * 64];                            \
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;              \
    if (i >= a.n) return;                                                 \
    const Strided blk = {blk_ + threadIdx.x, 64}, ws = {a.ws + i, a.n_pad};

template <class C> static __global__ __launch_bounds__(64) void shard_kernel(const Args a) {
    PRIO3_LANE
    const bool ok = shard_item<C>(a.t, a.measurement[i], a.rand + i * SEED * a.t.shares, a.leader + i * a.t.leader_words(), ws, blk);
    if (a.ok) a.ok[i] = ok;
}
template <class C> static __global__ __launch_bounds__(64) void prep_init_kernel(const Args a) {
    PRIO3_LANE
    const size_t row = a.agg_id == 0 ? (size_t)8 * a.t.leader_words() : (size_t)SEED;
    const bool ok = prep_init_item<C>(a.t, a.agg_id, a.verify_key, a.nonce + i * NONCE, a.share + i * row, a.prep_share + i * a.t.verifier_len(), a.out_share + i, ws, blk);
    if (a.ok) a.ok[i] = ok;
}
#undef PRIO3_LANE
template <class C> static __global__ __launch_bounds__(64) void prep_finish_kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    a.ok[i] = prep_finish_item<C>(a.t, reinterpret_cast<const uint64_t *>(a.share) + i * a.t.shares * a.t.verifier_len());
}

// AggregateUpdate over the batch: modular sums, so the order does not matter.  First launch: a grid-stride sum per thread, the
// wavefront's by shuffles, the workgroup's through LDS -> partial[blockIdx.x].  Second launch (one wavefront): agg += the partials.
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = fp64::add(v, (uint64_t)__shfl_down((unsigned long long)v, d, 64));
    return v;
}
static __global__ __launch_bounds__(AGG_THREADS) void aggregate_kernel(const uint64_t *out_share, const uint8_t *mask, size_t n, uint64_t *partial) {
    __shared__ uint64_t part[AGG_THREADS / 64];
    uint64_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * AGG_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * AGG_THREADS) {
        const uint64_t take = mask ? fp64::mask(mask[i] != 0) : ~uint64_t(0);
        acc = fp64::add(acc, fp64::canon(out_share[i]) & take);
    }
    acc = wave_sum(acc);
    if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < AGG_THREADS / 64; w++) acc = fp64::add(acc, part[w]);
        partial[blockIdx.x] = acc;
    }
}
static __global__ __launch_bounds__(64) void aggregate_finish_kernel(const uint64_t *partial, uint32_t blocks, uint64_t *agg_share) {
    uint64_t acc = 0;
    for (uint32_t i = threadIdx.x; i < blocks; i += 64) acc = fp64::add(acc, partial[i]);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *agg_share = fp64::add(fp64::canon(*agg_share), acc);
}
// The host forms' reduction: the out shares arrive as rows of `row` (the pipeline's items); one wavefront sums a row.
static __global__ __launch_bounds__(64) void aggregate_rows_kernel(const uint64_t *out_share, const uint8_t *mask, size_t row, uint64_t *sums) {
    const size_t base = (size_t)blockIdx.x * row;
    uint64_t acc = 0;
    for (size_t i = threadIdx.x; i < row; i += 64) {
        const uint64_t take = mask ? fp64::mask(mask[base + i] != 0) : ~uint64_t(0);
        acc = fp64::add(acc, fp64::canon(out_share[base + i]) & take);
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}
#endif

}  // namespace prio3
}  // namespace circl
