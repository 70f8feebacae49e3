// tests/hostsim/prio3_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/prio3_kernels.h, prio3_xof_dev.h and fp64_dev.h on the CPU (their host instantiation), so that the CPU-only test
// tier can check the very source the kernels are built from against the checker tests/prio3.py and the reference's vectors.  Nothing
// here is linked into libcirclhip.so.
//
// With -DPRIO3_HOSTSIM_MAIN it is a stand-alone program for a sanitizer build: every buffer is a heap block of exactly its size, a
// Count and a Sum batch run shard -> prep_init per aggregator -> prep_finish, and a tampered report must fail alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prio3_kernels.h"

using namespace circl;
using namespace circl::prio3;

namespace {

// a source of elements out of arrays, for Flp::query
struct ArraySrc {
    const uint64_t *rand, *share;
    void rand_begin() {}
    bool rand_next(uint64_t &e) { e = *rand++; return true; }
    void meas_begin() {}
    void proof_begin() {}
    bool next(uint64_t &e) { e = *share++; return true; }
};
// a stream of words out of an array, for sample()
struct WordSrc {
    const uint64_t *w;
    size_t left, used = 0;
    uint64_t next_word() {
        used++;
        if (!left) return ~uint64_t(0);
        left--;
        return *w++;
    }
};

struct Lane {
    std::vector<uint64_t> ws, blk;
    explicit Lane(const Task &t) : ws(t.ws_elems()), blk(RATE_WORDS) {}
    Strided w() { return Strided{ws.data(), 1}; }
    Strided b() { return Strided{blk.data(), 1}; }
};

}  // namespace

extern "C" {

size_t hs_prio3_task_size() { return sizeof(Task); }
int hs_prio3_task(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, Task *out) {
    if (!task_ok(kind, max_measurement) || shares < 2 || shares > 255 || ctx_len > (size_t)MAX_CTX) return -1;
    *out = make_task(kind, max_measurement, shares, ctx, ctx_len);
    return 0;
}
// leader_words, verifier_len, ws_elems, p, query_rand_len
void hs_prio3_sizes(const Task *t, uint32_t *out5) {
    out5[0] = t->leader_words(); out5[1] = t->verifier_len(); out5[2] = t->ws_elems(); out5[3] = t->p; out5[4] = t->query_rand_len();
}

void hs_prio3_shard(const Task *t, size_t n, const uint64_t *measurement, const uint8_t *rand, uint64_t *leader, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) {
        Lane l(*t);
        const uint8_t *r = rand + i * SEED * t->shares;
        uint64_t *row = leader + i * t->leader_words();
        ok[i] = t->kind == COUNT ? shard_item<CircuitCount>(*t, measurement[i], r, row, l.w(), l.b()) : shard_item<CircuitSum>(*t, measurement[i], r, row, l.w(), l.b());
    }
}

void hs_prio3_prep_init(const Task *t, uint32_t agg_id, const uint8_t *verify_key, size_t n, const uint8_t *nonce, const uint8_t *share, uint64_t *prep_share,
                        uint64_t *out_share, uint8_t *ok) {
    const size_t row = agg_id == 0 ? (size_t)8 * t->leader_words() : (size_t)SEED;
    for (size_t i = 0; i < n; i++) {
        Lane l(*t);
        uint64_t *ps = prep_share + i * t->verifier_len();
        ok[i] = t->kind == COUNT ? prep_init_item<CircuitCount>(*t, agg_id, verify_key, nonce + i * NONCE, share + i * row, ps, out_share + i, l.w(), l.b())
                                 : prep_init_item<CircuitSum>(*t, agg_id, verify_key, nonce + i * NONCE, share + i * row, ps, out_share + i, l.w(), l.b());
    }
}

void hs_prio3_prep_finish(const Task *t, size_t n, const uint64_t *prep_shares, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) {
        const uint64_t *row = prep_shares + i * t->shares * t->verifier_len();
        ok[i] = t->kind == COUNT ? prep_finish_item<CircuitCount>(*t, row) : prep_finish_item<CircuitSum>(*t, row);
    }
}

// Flp::query on elements given outright: rand[query_rand_len], share[leader_words] -> verifier[verifier_len], out; returns its verdict
int hs_prio3_query(const Task *t, const uint64_t *rand, const uint64_t *share, uint64_t *verifier, uint64_t *out) {
    Lane l(*t);
    ArraySrc src{rand, share};
    return t->kind == COUNT ? Flp<CircuitCount>::query(*t, l.w(), src, verifier, *out) : Flp<CircuitSum>::query(*t, l.w(), src, verifier, *out);
}

// op 0 add, 1 sub, 2 mul, 3 sqr (of a), 4 inv (of a)
void hs_fp64(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    for (size_t i = 0; i < n; i++)
        out[i] = op == 0 ? fp64::add(a[i], b[i]) : op == 1 ? fp64::sub(a[i], b[i]) : op == 2 ? fp64::mul(a[i], b[i]) : op == 3 ? fp64::sqr(a[i]) : fp64::inv(a[i]);
}

// the size-2^lg transform in place; inverse: the coefficients (scaled by 2^-lg)
void hs_prio3_ntt(uint32_t lg, uint64_t *v, int inverse) {
    if (inverse) intt(Strided{v, 1}, lg, fp64::inv_two_pow((int)lg));
    else ntt(Strided{v, 1}, lg);
}

// `count` elements out of a stream of nwords words; returns how many were sampled before the sampler gave up (count: none did),
// *used = the words it read
size_t hs_prio3_sample(const uint64_t *words, size_t nwords, uint64_t *out, size_t count, size_t *used) {
    WordSrc src{words, nwords};
    size_t k = 0;
    while (k < count && sample(src, out[k])) k++;
    *used = src.used;
    return k;
}

}  // extern "C"

#ifdef PRIO3_HOSTSIM_MAIN
namespace {

template <class T> struct Heap {   // a block of exactly its size
    T *p;
    size_t n;
    explicit Heap(size_t n) : p(new T[n]()), n(n) {}
    ~Heap() { delete[] p; }
    Heap(const Heap &) = delete;
};

bool flow(int kind, uint64_t max, int shares, size_t n) {
    const uint8_t ctx[] = "sanitizer run";
    Heap<Task> t(1);
    if (hs_prio3_task(kind, max, shares, ctx, sizeof ctx - 1, t.p)) return false;
    const size_t lw = t.p->leader_words(), vl = t.p->verifier_len();
    Heap<uint64_t> meas(n), leader(n * lw), prep(n * shares * vl), one(n * vl), out(n);
    Heap<uint8_t> rand(n * SEED * shares), nonce(n * NONCE), vk(SEED), ok(n), seeds(n * SEED);
    for (size_t i = 0; i < rand.n; i++) rand.p[i] = (uint8_t)(i * 131 + 7);
    for (size_t i = 0; i < nonce.n; i++) nonce.p[i] = (uint8_t)(i * 29 + 1);
    for (size_t i = 0; i < vk.n; i++) vk.p[i] = (uint8_t)(255 - i);
    for (size_t i = 0; i < n; i++) meas.p[i] = kind == COUNT ? i & 1 : (max / 3 + i) % (max + 1);
    hs_prio3_shard(t.p, n, meas.p, rand.p, leader.p, ok.p);
    for (size_t i = 0; i < n; i++)
        if (!ok.p[i]) return false;
    leader.p[lw * (n - 1) + lw - 1] ^= 1;   // the last report's proof share, tampered
    for (int j = 0; j < shares; j++) {
        if (j) for (size_t i = 0; i < n; i++) memcpy(seeds.p + i * SEED, rand.p + (i * shares + j - 1) * SEED, SEED);
        hs_prio3_prep_init(t.p, (uint32_t)j, vk.p, n, nonce.p, j ? seeds.p : reinterpret_cast<const uint8_t *>(leader.p), one.p, out.p, ok.p);
        for (size_t i = 0; i < n; i++) {
            if (!ok.p[i]) return false;
            memcpy(prep.p + (i * shares + j) * vl, one.p + i * vl, 8 * vl);
        }
    }
    hs_prio3_prep_finish(t.p, n, prep.p, ok.p);
    for (size_t i = 0; i < n; i++)
        if (ok.p[i] != (i + 1 < n)) return false;
    return true;
}

}  // namespace

int main() {
    const bool good = flow(COUNT, 0, 2, 3) && flow(COUNT, 0, 3, 2) && flow(SUM, 1, 2, 2) && flow(SUM, 255, 3, 3) && flow(SUM, 1337, 2, 2) &&
                      flow(SUM, (uint64_t(1) << 63) - 1, 2, 2);
    printf(good ? "prio3_hostsim: ok\n" : "prio3_hostsim: FAILED\n");
    return good ? 0 : 1;
}
#endif
