// api_prio3.hip -- batch Prio3Count and Prio3Sum (the reference's vdaf/prio3/count and /sum; draft-irtf-cfrg-vdaf-13 section 7) behind the
// C ABI (include/circl_hip.h): Shard, PrepInit, PrepSharesToPrep and AggregateUpdate over batches of reports under one task, one report
// per lane, and Unshard on the host.  No CPU compute path for the per-report work.
//
// Every entry point fills one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a host
// form) and goes through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// The task (kind, max_measurement, shares, ctx) is a parameter of every call; its context string is a HOST pointer in both forms and
// travels to the kernels by value inside the Task.  Measurements, rand, input shares, the verify key, out shares and the aggregate share
// are secret: the host forms wipe their page-locked staging and zero the device staging of every chunk, the per-report workspace
// included.  The launches run without a ProfScope: CIRCL_HIP_KERNEL_COUNT stays what it was.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
#include "prio3_kernels.h"
#include "host_compose.h"

#include <cstring>
#include <vector>

using namespace circl::host;
namespace p3 = circl::prio3;
namespace fp = circl::fp64;

namespace {

enum Op { SHARD, PREP_INIT, PREP_FINISH, AGGREGATE };

struct Call {
    Op op = SHARD;
    bool task_valid = false;
    p3::Task t;
    int agg_id = 0;
    const uint64_t *measurement = nullptr;
    const uint8_t *rand = nullptr, *verify_key = nullptr, *nonce = nullptr, *share = nullptr, *mask = nullptr;
    uint8_t *leader = nullptr, *prep_share = nullptr, *out_share = nullptr, *ok = nullptr;
    uint8_t *agg = nullptr;        // AGGREGATE: the aggregate share (_dev), or the rows' sums (the host form's launches)
    size_t agg_rows = 0;           // AGGREGATE through the host pipeline: n is a count of rows of AGG_ROW out shares
    uint8_t *ws = nullptr;
    size_t ws_bytes = 0;
    size_t n = 0;
};

constexpr size_t AGG_WS = size_t(8) * p3::AGG_BLOCKS;   // the reduction's partial sums
constexpr size_t AGG_ROW = 4096;                        // out shares per row of the host form's reduction

bool task_args_ok(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len) {
    return p3::task_ok(kind, max_measurement) && shares >= 2 && shares <= 255 && ctx_len <= (size_t)p3::MAX_CTX && (ctx || ctx_len == 0);
}
void set_task(Call &c, int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len) {
    c.task_valid = task_args_ok(kind, max_measurement, shares, ctx, ctx_len);
    if (c.task_valid) c.t = p3::make_task(kind, max_measurement, shares, ctx, ctx_len);
    else memset(&c.t, 0, sizeof c.t);
}

size_t n_pad(size_t n) { return (n + 63) & ~size_t(63); }
// what the per-report kernels of task t need for n reports
size_t lane_ws_bytes(const p3::Task &t, size_t n) { return up256(size_t(8) * t.ws_elems() * n_pad(n)); }
size_t ws_need(const Call &c) { return c.op == AGGREGATE ? (c.agg_rows ? 0 : AGG_WS) : c.op == PREP_FINISH ? 0 : lane_ws_bytes(c.t, c.n); }

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (!c.task_valid) return CIRCL_HIP_EPARAM;
    if (c.op == PREP_INIT && (c.agg_id < 0 || (uint32_t)c.agg_id >= c.t.shares)) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    switch (c.op) {
        case SHARD: return c.measurement && c.rand && c.leader ? CIRCL_HIP_OK : CIRCL_HIP_EPARAM;
        case PREP_INIT: return c.verify_key && c.nonce && c.share && c.prep_share && c.out_share ? CIRCL_HIP_OK : CIRCL_HIP_EPARAM;
        case PREP_FINISH: return c.share && c.ok ? CIRCL_HIP_OK : CIRCL_HIP_EPARAM;
        case AGGREGATE: return c.out_share && c.agg ? CIRCL_HIP_OK : CIRCL_HIP_EPARAM;
    }
    return CIRCL_HIP_EPARAM;
}

template <class C> void launch_lanes(const Call &c, const p3::Args &a, hipStream_t st) {
    const dim3 grid = lanes_grid(c.n), block(64);
    if (c.op == SHARD) hipLaunchKernelGGL((p3::shard_kernel<C>), grid, block, 0, st, a);
    else if (c.op == PREP_INIT) hipLaunchKernelGGL((p3::prep_init_kernel<C>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((p3::prep_finish_kernel<C>), grid, block, 0, st, a);
}

// the launches of one call on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<8>(c.measurement, c.rand, c.verify_key, c.nonce, c.share, c.leader, c.prep_share, c.out_share, c.agg, c.ws)) return CIRCL_HIP_EWORKSPACE;
    const size_t need = ws_need(c);
    if (need && (!c.ws || c.ws_bytes < need)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (c.op == AGGREGATE) {
        const uint64_t *in = reinterpret_cast<const uint64_t *>(c.out_share);
        uint64_t *agg = reinterpret_cast<uint64_t *>(c.agg);
        if (c.agg_rows) {
            hipLaunchKernelGGL(p3::aggregate_rows_kernel, dim3((unsigned)c.agg_rows), dim3(64), 0, st, in, c.mask, AGG_ROW, agg);
        } else {
            uint64_t *partial = reinterpret_cast<uint64_t *>(c.ws);
            const size_t want = (c.n + p3::AGG_THREADS - 1) / p3::AGG_THREADS;
            const unsigned blocks = (unsigned)(want < (size_t)p3::AGG_BLOCKS ? want : (size_t)p3::AGG_BLOCKS);
            hipLaunchKernelGGL(p3::aggregate_kernel, dim3(blocks), dim3(p3::AGG_THREADS), 0, st, in, c.mask, c.n, partial);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(p3::aggregate_finish_kernel, dim3(1), dim3(64), 0, st, partial, blocks, agg);
        }
        HIP_TRY(hipGetLastError());
        return CIRCL_HIP_OK;
    }
    p3::Args a = {};
    a.t = c.t;
    a.agg_id = (uint32_t)c.agg_id;
    a.measurement = c.measurement;
    a.rand = c.rand;
    a.verify_key = c.verify_key;
    a.nonce = c.nonce;
    a.share = c.share;
    a.leader = reinterpret_cast<uint64_t *>(c.leader);
    a.prep_share = reinterpret_cast<uint64_t *>(c.prep_share);
    a.out_share = reinterpret_cast<uint64_t *>(c.out_share);
    a.ok = c.ok;
    a.ws = reinterpret_cast<uint64_t *>(c.ws);
    a.n = c.n;
    a.n_pad = n_pad(c.n);
    if (c.t.kind == (uint32_t)p3::COUNT) launch_lanes<p3::CircuitCount>(c, a, st);
    else launch_lanes<p3::CircuitSum>(c, a, st);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int pipeline(const Call &c, size_t n, int device, size_t chunk) {
    const PipeOpts opts = secret_opts(chunk);
    const size_t leader = size_t(8) * c.t.leader_words(), prep = size_t(8) * c.t.verifier_len();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        switch (c.op) {
            case SHARD:
                b.rows(&Call::measurement, 8, true);
                b.rows(&Call::rand, size_t(p3::SEED) * c.t.shares, true);
                b.out(&Call::leader, leader, true);
                b.out(&Call::ok, 1, false);
                break;
            case PREP_INIT:
                b.rows(&Call::verify_key, p3::SEED, true, true);
                b.rows(&Call::nonce, p3::NONCE, false);
                b.rows(&Call::share, c.agg_id == 0 ? leader : size_t(p3::SEED), true);
                b.out(&Call::prep_share, prep, false);
                b.out(&Call::out_share, 8, true);
                b.out(&Call::ok, 1, false);
                break;
            case PREP_FINISH:
                b.rows(&Call::share, prep * c.t.shares, false);
                b.out(&Call::ok, 1, false);
                break;
            case AGGREGATE:   // rows of AGG_ROW out shares, one sum per row
                b.rows(&Call::out_share, 8 * AGG_ROW, true);
                b.rows(&Call::mask, AGG_ROW, false);
                b.out(&Call::agg, 8, true);
                break;
        }
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, [&](size_t k) { Call d = c; d.n = k; return ws_need(d); }, opts, [&](Chunk &k) {
            Call d = b.on(k);
            d.ws = k.ws;
            d.ws_bytes = k.ws_bytes;
            if (c.op == AGGREGATE) d.agg_rows = k.cnt;
            return launch(d, k.st);
        });
    }, kHeavyOneDeviceMax);
}

// AggregateUpdate from host memory: the out shares go through the pipeline as rows of AGG_ROW (the last one padded here, its padding
// masked off), a launch sums every row, and the few row sums -- one per 4096 reports -- are added to the aggregate share here.
int host_aggregate(const Call &caller, int device) {
    const size_t n = caller.n, full = n / AGG_ROW, tail = n % AGG_ROW;
    std::vector<uint64_t> sums(full + (tail ? 1 : 0));
    int rc = CIRCL_HIP_OK;
    if (full) {
        Call c = caller;
        c.agg_rows = c.n = full;
        c.agg = reinterpret_cast<uint8_t *>(sums.data());
        rc = pipeline(c, full, device, 64);
    }
    if (rc == CIRCL_HIP_OK && tail) {
        std::vector<uint64_t> row(AGG_ROW, 0);
        std::vector<uint8_t> mask(AGG_ROW, 0);
        memcpy(row.data(), caller.out_share + 8 * AGG_ROW * full, 8 * tail);
        for (size_t i = 0; i < tail; i++) mask[i] = caller.mask ? caller.mask[AGG_ROW * full + i] : 1;
        Call c = caller;
        c.agg_rows = c.n = 1;
        c.out_share = reinterpret_cast<uint8_t *>(row.data());
        c.mask = mask.data();
        c.agg = reinterpret_cast<uint8_t *>(sums.data() + full);
        rc = pipeline(c, 1, device, 64);
        volatile uint64_t *w = row.data();
        for (size_t i = 0; i < AGG_ROW; i++) w[i] = 0;
    }
    if (rc == CIRCL_HIP_OK) {
        uint64_t acc;
        memcpy(&acc, caller.agg, 8);
        acc = fp::canon(acc);
        for (uint64_t s : sums) acc = fp::add(acc, s);
        memcpy(caller.agg, &acc, 8);
    }
    volatile uint64_t *w = sums.data();
    for (size_t i = 0; i < sums.size(); i++) w[i] = 0;
    return rc;
}

int host_pipeline(const Call &c, int device) {
    if (c.op == AGGREGATE) return host_aggregate(c, device);
    return pipeline(c, c.n, device, c.t.p >= 64 ? size_t(1) << 13 : size_t(1) << 15);
}

}  // namespace

// both forms of an entry point whose _dev form takes a workspace: NAME(params..., n, int device) and
// NAME_dev(params..., n, void *d_workspace, size_t workspace_bytes, void *stream)
#define WS_FORMS(NAME, PARAMS, BODY)                                                                  \
    int NAME(PARAMS, size_t n, int device) {                                                          \
        const bool dev_ = false;                                                                      \
        void *stream = nullptr, *d_workspace = nullptr;                                               \
        const size_t workspace_bytes = 0;                                                             \
        BODY                                                                                          \
    }                                                                                                 \
    int NAME##_dev(PARAMS, size_t n, void *d_workspace, size_t workspace_bytes, void *stream) {       \
        const bool dev_ = true;                                                                       \
        const int device = 0;                                                                         \
        BODY                                                                                          \
    }
#define TASK_PARAMS int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len
#define TASK_ARGS kind, max_measurement, shares, ctx, ctx_len

extern "C" {

size_t circl_hip_prio3_leader_share_size(int kind, uint64_t max_measurement) {
    if (!p3::task_ok(kind, max_measurement)) return 0;
    return size_t(8) * p3::make_task(kind, max_measurement, 2, nullptr, 0).leader_words();
}
size_t circl_hip_prio3_prep_share_size(int kind) { return kind == p3::COUNT ? 32 : kind == p3::SUM ? 24 : 0; }
size_t circl_hip_prio3_rand_size(int shares) { return shares >= 2 && shares <= 255 ? size_t(p3::SEED) * shares : 0; }
size_t circl_hip_prio3_workspace_size(int kind, uint64_t max_measurement, size_t n) {
    if (!p3::task_ok(kind, max_measurement)) return 0;
    const size_t lanes = lane_ws_bytes(p3::make_task(kind, max_measurement, 2, nullptr, 0), n);
    return lanes > AGG_WS ? lanes : AGG_WS;
}

WS_FORMS(circl_hip_prio3_shard, P(TASK_PARAMS, const uint64_t *measurement, const uint8_t *rand, uint8_t *leader_share, uint8_t *ok), {
    Call c;
    c.op = SHARD;
    set_task(c, TASK_ARGS);
    c.measurement = measurement; c.rand = rand; c.leader = leader_share; c.ok = ok; c.n = n;
    c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run_call(c, dev_, device, stream);
})

WS_FORMS(circl_hip_prio3_prep_init,
         P(TASK_PARAMS, int agg_id, const uint8_t *verify_key, const uint8_t *nonce, const uint8_t *input_share, uint8_t *prep_share, uint8_t *out_share, uint8_t *ok), {
             Call c;
             c.op = PREP_INIT;
             set_task(c, TASK_ARGS);
             c.agg_id = agg_id; c.verify_key = verify_key; c.nonce = nonce; c.share = input_share; c.prep_share = prep_share; c.out_share = out_share; c.ok = ok; c.n = n;
             c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
             return run_call(c, dev_, device, stream);
         })

BOTH_FORMS(circl_hip_prio3_prep_finish, P(TASK_PARAMS, const uint8_t *prep_shares, uint8_t *ok), {
    Call c;
    c.op = PREP_FINISH;
    set_task(c, TASK_ARGS);
    c.share = prep_shares; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

WS_FORMS(circl_hip_prio3_aggregate, P(TASK_PARAMS, const uint8_t *out_share, const uint8_t *mask, uint8_t *agg_share), {
    Call c;
    c.op = AGGREGATE;
    set_task(c, TASK_ARGS);
    c.out_share = const_cast<uint8_t *>(out_share); c.mask = mask; c.agg = agg_share; c.n = n;
    c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run_call(c, dev_, device, stream);
})

int circl_hip_prio3_unshard(TASK_PARAMS, const uint8_t *agg_shares, uint64_t num_measurements, uint64_t *result) {
    if (!task_args_ok(TASK_ARGS) || !agg_shares || !result) return CIRCL_HIP_EPARAM;
    if (kind == p3::SUM) {   // the reference's ErrAggregateBound: num_measurements * max_measurement must be an element
        const uint64_t hi = fp::mulhi(num_measurements, max_measurement), lo = num_measurements * max_measurement;
        if (hi || !fp::canonical(lo)) return CIRCL_HIP_EPARAM;
    }
    uint64_t acc = 0;
    for (int j = 0; j < shares; j++) {
        uint64_t e;
        memcpy(&e, agg_shares + 8 * j, 8);
        if (!fp::canonical(e)) return CIRCL_HIP_EPARAM;
        acc = fp::add(acc, e);
    }
    *result = acc;
    return CIRCL_HIP_OK;
}

}  // extern "C"
