// api_dleq.hip -- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms; RFC 9497 section 2.2) on ristretto255 and the mode-2 (POPRF) item
// operations of oprf/client.go and oprf/server.go behind the C ABI (include/circl_hip.h).  No CPU compute path.
//
// As in api_oprf.hip every entry point fills one Call and goes through check() -- the argument contract, before any device is looked
// for -- and then launch() or host_pipeline().  The proofs' item is the REQUEST: the pipeline and shard split on requests, the element
// arrays travel as blobs over ONE scaled copy of req_off (x 32 bytes) that is built once per call, and a launch gets the chunk's
// offsets in bytes (dleq::Args::off_shift).  k and r are secret: their staging is wiped and the device staging of every chunk is zeroed,
// except the workspace, which holds sums of public points only.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
#include "dleq_kernels.h"
#include "host_compose.h"

using namespace circl::host;
namespace dq = circl::dleq;

namespace {

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *w(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

constexpr size_t kMaxCtx = 255 - dq::kTagHead;   // "HashToScalar-" || dst must fit xmd's tag

// ---- the proofs ----------------------------------------------------------------------------------------------------------------
struct Call {
    bool verify = false;
    const uint8_t *k = nullptr, *kA = nullptr, *B = nullptr, *kB = nullptr, *r = nullptr, *dst = nullptr;
    size_t k_stride = 32, kA_stride = 32, dst_len = 0;
    const uint64_t *off = nullptr;
    uint32_t off_shift = 0, flags = 0;
    uint8_t *proofs = nullptr, *ok = nullptr;   // verify reads the proofs
    size_t n_req = 0, n_elems = 0;
    uint8_t *ws = nullptr;
    size_t ws_bytes = 0;
};

size_t slots(size_t n_req, size_t n_elems) { return (n_elems + 63) / 64 + n_req; }
size_t ws_size(size_t n_req, size_t n_elems) { return up256(4 * n_req) + up256(slots(n_req, n_elems) * 2 * dq::PW * 4); }

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (c.kA_stride != 0 && c.kA_stride != 32) return CIRCL_HIP_EPARAM;
    if (!c.verify && c.k_stride != 0 && c.k_stride != 32) return CIRCL_HIP_EPARAM;
    if (c.dst_len > kMaxCtx || (c.dst_len && !c.dst)) return CIRCL_HIP_EPARAM;
    if (c.flags & ~dq::kNoIdentity) return CIRCL_HIP_EPARAM;
    if (c.n_req == 0) return CIRCL_HIP_OK;
    if (!c.kA || !c.B || !c.kB || !c.off || !c.proofs) return CIRCL_HIP_EPARAM;
    if (c.verify ? !c.ok : (!c.k || !c.r)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

// two launches on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.k, c.kA, c.B, c.kB, c.r, c.proofs) || !aligned<8>(c.off) || !aligned<8>(c.ws)) return CIRCL_HIP_EWORKSPACE;
    if (!c.ws || c.ws_bytes < ws_size(c.n_req, c.n_elems)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    dq::Args a = {};
    a.off = c.off;
    a.off_shift = c.off_shift;
    a.B = w(c.B);
    a.kB = w(c.kB);
    a.k = w(c.k);
    a.k_stride = c.k_stride / 4;
    a.kA = w(c.kA);
    a.kA_stride = c.kA_stride / 4;
    a.r = w(c.r);
    a.proofs = w(c.proofs);
    a.ok = c.ok;
    a.bad = w(c.ws);
    a.partial = w(c.ws + up256(4 * c.n_req));
    a.n_req = c.n_req;
    a.n_elems = c.n_elems;
    a.flags = c.flags;
    memcpy(a.tag, "HashToScalar-", dq::kTagHead);
    if (c.dst_len) memcpy(a.tag + dq::kTagHead, c.dst, c.dst_len);
    a.tag_len = (uint32_t)(dq::kTagHead + c.dst_len);
    HIP_TRY(hipMemsetAsync(a.bad, 0, 4 * c.n_req, st));
    if (c.n_elems) {
        ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_COMPOSITE, st);
        if (c.verify) hipLaunchKernelGGL(dq::composite<true>, lanes_grid(c.n_elems), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(dq::composite<false>, lanes_grid(c.n_elems), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_FINISH, st);
    if (c.verify) hipLaunchKernelGGL(dq::finish<true>, lanes_grid(c.n_req), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(dq::finish<false>, lanes_grid(c.n_req), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host form: shard / run_pipeline over requests --------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    // the one scaled copy of the offsets: the element arrays are blobs of 32-byte rows, staged from the call that holds it
    std::vector<uint64_t> scaled(c.n_req + 1);
    for (size_t g = 0; g <= c.n_req; g++) scaled[g] = c.off[g] * 32;
    Call sc = c;
    sc.off = scaled.data();
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 14);
    opts.wipe_device = !c.verify;
    opts.ws_secret_bytes = [](size_t) { return size_t(0); };   // partial sums of d_j B_j: public
    return shard(c.n_req, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(sc, lo, &Call::n_req);
        b.rows(&Call::kA, 32, false, c.kA_stride == 0);
        b.rows(&Call::k, 32, true, c.k_stride == 0, !c.verify);
        b.rows(&Call::r, 32, true, false, !c.verify);
        if (c.verify) b.rows(&Call::proofs, 64, false);
        else b.out(&Call::proofs, 64, false);
        b.blob(&Call::B, &Call::off, false);
        b.blob(&Call::kB, &Call::off, false);    // (each blob stages the offsets; a launch reads one copy)
        b.out(&Call::ok, 1, false);
        // a chunk's workspace: sized for the chunk of this shard that has the most elements
        const size_t chunk = std::max<size_t>(1, std::min(cnt, opts.chunk_items));
        size_t most = 0;
        for (size_t s = lo; s < lo + cnt; s += chunk) most = std::max<size_t>(most, c.off[std::min(s + chunk, lo + cnt)] - c.off[s]);
        size_t at = lo;   // the chunks of a shard are launched in order, on this thread
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, [&](size_t n) { return ws_size(n, most); }, opts, [&](Chunk &k) {
            Call d = b.on(k);
            d.off_shift = 5;
            d.n_elems = c.off[at + k.cnt] - c.off[at];
            at += k.cnt;
            d.ws = k.ws;
            d.ws_bytes = k.ws_bytes;
            return launch(d, k.st);
        });
    }, kHeavyOneDeviceMax);
}

int run(Call &c, bool dev, int device, void *stream) {
    if (int rc = check(c)) return rc;
    if (c.n_req == 0) return CIRCL_HIP_OK;
    if (dev) return launch(c, static_cast<hipStream_t>(stream));
    if (c.off[0] != 0) return CIRCL_HIP_EPARAM;
    for (size_t g = 0; g < c.n_req; g++)
        if (c.off[g + 1] < c.off[g]) return CIRCL_HIP_EPARAM;
    c.n_elems = c.off[c.n_req];
    return host_pipeline(c, device);
}

// ---- the POPRF items: one item per lane, one launch per call, no workspace ----------------------------------------------------------
struct ItemCall {
    int op = dq::kTweakServer;
    const uint8_t *input = nullptr, *info = nullptr, *scalars = nullptr, *elems = nullptr;
    const uint64_t *input_off = nullptr, *info_off = nullptr;
    size_t scalar_stride = 32, elem_stride = 32;
    uint8_t *out = nullptr, *out2 = nullptr, *out3 = nullptr, *ok = nullptr;
    size_t n = 0;

    bool takes_input() const { return op == dq::kPoprfFinalize || op == dq::kPoprfFullEvaluate; }
    bool takes_scalars() const { return op != dq::kTweakClient; }
    bool takes_elems() const { return op == dq::kTweakClient || op == dq::kPoprfFinalize; }
    size_t out_row() const { return takes_input() ? 64 : 32; }
};

int check(const ItemCall &c) {
    if (c.scalar_stride != 0 && c.scalar_stride != 32) return CIRCL_HIP_EPARAM;
    if (c.elem_stride != 0 && c.elem_stride != 32) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == dq::kTweakServer && (!c.out2 || !c.out3))) return CIRCL_HIP_EPARAM;
    if (c.takes_scalars() && !c.scalars) return CIRCL_HIP_EPARAM;
    if (c.takes_elems() && !c.elems) return CIRCL_HIP_EPARAM;
    if ((c.input && !c.input_off) || (c.info && !c.info_off)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

constexpr int kItemKernelId[dq::kItemOps] = {CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_FINALIZE,
                                             CIRCL_HIP_KERNEL_OPRF_POPRF_FULL_EVALUATE};

int launch(const ItemCall &c, hipStream_t st) {
    if (!aligned<4>(c.scalars, c.elems, c.out, c.out2, c.out3) || !aligned<8>(c.input_off, c.info_off)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    dq::ItemArgs a = {};
    a.input = c.takes_input() ? c.input : nullptr;
    a.input_off = a.input ? c.input_off : nullptr;
    a.info = c.info;
    a.info_off = a.info ? c.info_off : nullptr;
    a.scalars = w(c.scalars);
    a.scalar_stride = c.scalar_stride / 4;
    a.elems = w(c.elems);
    a.elem_stride = c.elem_stride / 4;
    a.out = w(c.out);
    a.out2 = w(c.out2);
    a.out3 = w(c.out3);
    a.ok = c.ok;
    a.n = c.n;
    const dim3 grid = lanes_grid(c.n), block(64);
    ProfScope ps(kItemKernelId[c.op], st);
    switch (c.op) {
#define DLEQ_ITEM_LAUNCH(OP) case dq::OP: hipLaunchKernelGGL(dq::item_kernel<dq::OP>, grid, block, 0, st, a); break
        DLEQ_ITEM_LAUNCH(kTweakServer);
        DLEQ_ITEM_LAUNCH(kTweakClient);
        DLEQ_ITEM_LAUNCH(kPoprfFinalize);
        DLEQ_ITEM_LAUNCH(kPoprfFullEvaluate);
#undef DLEQ_ITEM_LAUNCH
        default: return CIRCL_HIP_EPARAM;
    }
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int host_pipeline(const ItemCall &c, int device) {
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<ItemCall> b(c, lo);
        b.rows(&ItemCall::scalars, 32, true, c.scalar_stride == 0, c.takes_scalars());
        b.rows(&ItemCall::elems, 32, false, c.op == dq::kTweakClient && c.elem_stride == 0, c.takes_elems());
        b.blob(&ItemCall::input, &ItemCall::input_off, true, 0, c.takes_input());   // the client's private input
        b.blob(&ItemCall::info, &ItemCall::info_off, false);
        b.out(&ItemCall::out, c.out_row(), c.op != dq::kTweakClient);
        b.out(&ItemCall::out2, 32, true, c.op == dq::kTweakServer);
        b.out(&ItemCall::out3, 32, false, c.op == dq::kTweakServer);
        b.out(&ItemCall::ok, 1, false);
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

// sk given: the server's side (t, t^-1, t G); pkS given: the client's (the tweaked key only); both or neither: no call
int run_tweak(ItemCall &c, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, bool dev, int device, void *stream) {
    if ((sk != nullptr) == (pkS != nullptr)) return CIRCL_HIP_EPARAM;
    c.op = sk ? dq::kTweakServer : dq::kTweakClient;
    c.scalars = sk;
    c.scalar_stride = sk_stride;
    c.elems = pkS;
    c.elem_stride = pk_stride;
    if (!sk) {
        c.out = c.out3;
        c.out2 = c.out3 = nullptr;
    }
    return run_call(c, dev, device, stream);
}

}  // namespace

#define DLEQ_PARAMS_ const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off
#define DLEQ_TAIL_ const uint8_t *dst, size_t dst_len, uint32_t flags

extern "C" {

size_t circl_hip_dleq_workspace_size(size_t n_req, size_t n_elems) { return ws_size(n_req, n_elems); }

#define DLEQ_FILL(VERIFY)                                                                                                                  \
    Call c;                                                                                                                                \
    c.verify = VERIFY; c.kA = kA; c.kA_stride = kA_stride; c.B = B; c.kB = kB; c.off = req_off; c.dst = dst; c.dst_len = dst_len;           \
    c.flags = flags; c.ok = ok; c.n_req = n_req;

int circl_hip_dleq_prove(const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req, int device) {
    DLEQ_FILL(false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    return run(c, false, device, nullptr);
}
int circl_hip_dleq_prove_dev(const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req,
                             size_t n_elems, void *d_workspace, size_t workspace_bytes, void *stream) {
    DLEQ_FILL(false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}
int circl_hip_dleq_verify(DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, int device) {
    DLEQ_FILL(true)
    c.proofs = const_cast<uint8_t *>(proofs);
    return run(c, false, device, nullptr);
}
int circl_hip_dleq_verify_dev(DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, size_t n_elems, void *d_workspace,
                              size_t workspace_bytes, void *stream) {
    DLEQ_FILL(true)
    c.proofs = const_cast<uint8_t *>(proofs);
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}

BOTH_FORMS(circl_hip_oprf_poprf_tweak,
           P(const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *t,
             uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok),
           {
               ItemCall c;
               c.info = info_blob; c.info_off = info_off; c.out = t; c.out2 = t_inv; c.out3 = tweaked; c.ok = ok; c.n = n;
               return run_tweak(c, sk, sk_stride, pkS, pk_stride, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_poprf_finalize,
           P(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off, const uint8_t *blinds,
             const uint8_t *evaluated, uint8_t *out, uint8_t *ok),
           {
               ItemCall c;
               c.op = dq::kPoprfFinalize; c.input = input_blob; c.input_off = input_off; c.info = info_blob; c.info_off = info_off; c.scalars = blinds;
               c.elems = evaluated; c.out = out; c.ok = ok; c.n = n;
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_poprf_full_evaluate,
           P(const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off,
             uint8_t *out, uint8_t *ok),
           {
               ItemCall c;
               c.op = dq::kPoprfFullEvaluate; c.scalars = sk; c.scalar_stride = sk_stride; c.input = input_blob; c.input_off = input_off;
               c.info = info_blob; c.info_off = info_off; c.out = out; c.ok = ok; c.n = n;
               return run_call(c, dev_, device, stream);
           })

}  // extern "C"
