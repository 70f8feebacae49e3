// api_dleq_nistp.hip -- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms; RFC 9497 section 2.2) on P-256 and P-384 and the mode-2
// (POPRF) item operations of oprf/client.go and oprf/server.go for suites P256-SHA256 and P384-SHA384, behind the C ABI
// (include/circl_hip.h).  No CPU compute path.  The kernels are dleq_group_kernels.h's, instantiated for the two curves here and
// nowhere else: the NIST field code is expensive to compile, and a unit of its own keeps that off the other units' build.
//
// The shape is api_dleq.hip's: every entry point fills one Call and goes through check() -- the argument contract, before any device is
// looked for -- and then launch() or host_pipeline().  The proofs' item is the REQUEST: the pipeline and shard split on requests, the
// element arrays travel as blobs over ONE scaled copy of req_off (x Ne bytes) that is built once per call, and a launch gets the
// chunk's offsets in bytes with the divisor Ne (gdleq::Args::off_div).  k and r are secret: their staging is wiped and the device
// staging of every chunk is zeroed, except the workspace, which holds sums of public points only.
#include "dleq_group_kernels.h"
#include "host_compose.h"

using namespace circl::host;
namespace gq = circl::gdleq;
using circl::oprf::P256;
using circl::oprf::P384;

namespace {

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *w(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

constexpr size_t kMaxCtx = 255 - gq::kTagHead;   // "HashToScalar-" || dst must fit xmd's tag

// the rows of a curve: a scalar, an element, an OPRF output, the words of a point in the workspace; ns = 0: no such curve
struct Dims {
    size_t ns = 0, ne = 0, nh = 0, pw = 0;
};
template <class G> constexpr Dims dims_of() { return {G::NS, G::NE, G::NH, gq::Ops<G>::PW}; }
Dims dims(int curve) { return curve == CIRCL_HIP_P256 ? dims_of<P256>() : curve == CIRCL_HIP_P384 ? dims_of<P384>() : Dims(); }

// ---- the proofs ----------------------------------------------------------------------------------------------------------------
struct Call {
    int curve = 0;
    bool verify = false;
    const uint8_t *k = nullptr, *kA = nullptr, *B = nullptr, *kB = nullptr, *r = nullptr, *dst = nullptr;
    size_t k_stride = 0, kA_stride = 0, dst_len = 0;
    const uint64_t *off = nullptr;
    uint32_t off_div = 1, flags = 0;
    uint8_t *proofs = nullptr, *ok = nullptr;   // verify reads the proofs
    size_t n_req = 0, n_elems = 0;
    uint8_t *ws = nullptr;
    size_t ws_bytes = 0;
};

size_t slots(size_t n_req, size_t n_elems) { return (n_elems + 63) / 64 + n_req; }
size_t ws_size(const Dims &d, size_t n_req, size_t n_elems) { return up256(4 * n_req) + up256(slots(n_req, n_elems) * 2 * d.pw * 4); }

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    const Dims d = dims(c.curve);
    if (!d.ns) return CIRCL_HIP_EPARAM;
    if (c.kA_stride != 0 && c.kA_stride != d.ne) return CIRCL_HIP_EPARAM;
    if (!c.verify && c.k_stride != 0 && c.k_stride != d.ns) return CIRCL_HIP_EPARAM;
    if (c.dst_len > kMaxCtx || (c.dst_len && !c.dst)) return CIRCL_HIP_EPARAM;
    if (c.flags & ~gq::kNoIdentity) return CIRCL_HIP_EPARAM;
    if (c.n_req == 0) return CIRCL_HIP_OK;
    if (!c.kA || !c.B || !c.kB || !c.off || !c.proofs) return CIRCL_HIP_EPARAM;
    if (c.verify ? !c.ok : (!c.k || !c.r)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

template <class G> void launch_composite(const Call &c, const gq::Args &a, hipStream_t st) {
    if (c.verify) hipLaunchKernelGGL((gq::composite<G, true>), lanes_grid(c.n_elems), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((gq::composite<G, false>), lanes_grid(c.n_elems), dim3(64), 0, st, a);
}
template <class G> void launch_finish(const Call &c, const gq::Args &a, hipStream_t st) {
    if (c.verify) hipLaunchKernelGGL((gq::finish<G, true>), lanes_grid(c.n_req), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((gq::finish<G, false>), lanes_grid(c.n_req), dim3(64), 0, st, a);
}

// two launches on device pointers.  Scalar and proof rows are words; element rows (kA, B, kB) are bytes and may lie anywhere.
int launch(const Call &c, hipStream_t st) {
    const Dims d = dims(c.curve);
    if (!aligned<4>(c.k, c.r, c.proofs) || !aligned<8>(c.off) || !aligned<8>(c.ws)) return CIRCL_HIP_EWORKSPACE;
    if (!c.ws || c.ws_bytes < ws_size(d, c.n_req, c.n_elems)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    gq::Args a = {};
    a.off = c.off;
    a.off_div = c.off_div;
    a.B = c.B;
    a.kB = c.kB;
    a.k = w(c.k);
    a.k_stride = c.k_stride / 4;
    a.kA = c.kA;
    a.kA_stride = c.kA_stride;
    a.r = w(c.r);
    a.proofs = w(c.proofs);
    a.ok = c.ok;
    a.bad = w(c.ws);
    a.partial = w(c.ws + up256(4 * c.n_req));
    a.n_req = c.n_req;
    a.n_elems = c.n_elems;
    a.flags = c.flags;
    memcpy(a.tag, "HashToScalar-", gq::kTagHead);
    if (c.dst_len) memcpy(a.tag + gq::kTagHead, c.dst, c.dst_len);
    a.tag_len = (uint32_t)(gq::kTagHead + c.dst_len);
    HIP_TRY(hipMemsetAsync(a.bad, 0, 4 * c.n_req, st));
    if (c.n_elems) {
        ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_COMPOSITE, st);
        if (c.curve == CIRCL_HIP_P256) launch_composite<P256>(c, a, st);
        else launch_composite<P384>(c, a, st);
        HIP_TRY(hipGetLastError());
    }
    ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_FINISH, st);
    if (c.curve == CIRCL_HIP_P256) launch_finish<P256>(c, a, st);
    else launch_finish<P384>(c, a, st);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host form: shard / run_pipeline over requests --------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    const Dims d = dims(c.curve);
    // the one scaled copy of the offsets: the element arrays are blobs of Ne-byte rows, staged from the call that holds it
    std::vector<uint64_t> scaled(c.n_req + 1);
    for (size_t g = 0; g <= c.n_req; g++) scaled[g] = c.off[g] * d.ne;
    Call sc = c;
    sc.off = scaled.data();
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 14);
    opts.wipe_device = !c.verify;
    opts.ws_secret_bytes = [](size_t) { return size_t(0); };   // partial sums of d_j B_j: public
    return shard(c.n_req, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(sc, lo, &Call::n_req);
        b.rows(&Call::kA, d.ne, false, c.kA_stride == 0);
        b.rows(&Call::k, d.ns, true, c.k_stride == 0, !c.verify);
        b.rows(&Call::r, d.ns, true, false, !c.verify);
        if (c.verify) b.rows(&Call::proofs, 2 * d.ns, false);
        else b.out(&Call::proofs, 2 * d.ns, false);
        b.blob(&Call::B, &Call::off, false);
        b.blob(&Call::kB, &Call::off, false);    // (each blob stages the offsets; a launch reads one copy)
        b.out(&Call::ok, 1, false);
        // a chunk's workspace: sized for the chunk of this shard that has the most elements
        const size_t chunk = std::max<size_t>(1, std::min(cnt, opts.chunk_items));
        size_t most = 0;
        for (size_t s = lo; s < lo + cnt; s += chunk) most = std::max<size_t>(most, c.off[std::min(s + chunk, lo + cnt)] - c.off[s]);
        size_t at = lo;   // the chunks of a shard are launched in order, on this thread
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, [&](size_t n) { return ws_size(d, n, most); }, opts, [&](Chunk &k) {
            Call dc = b.on(k);
            dc.off_div = (uint32_t)d.ne;
            dc.n_elems = c.off[at + k.cnt] - c.off[at];
            at += k.cnt;
            dc.ws = k.ws;
            dc.ws_bytes = k.ws_bytes;
            return launch(dc, k.st);
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
    int curve = 0, op = gq::kTweakServer;
    const uint8_t *input = nullptr, *info = nullptr, *scalars = nullptr, *elems = nullptr;
    const uint64_t *input_off = nullptr, *info_off = nullptr;
    size_t scalar_stride = 0, elem_stride = 0;
    uint8_t *out = nullptr, *out2 = nullptr, *out3 = nullptr, *ok = nullptr;
    size_t n = 0;

    bool takes_input() const { return op == gq::kPoprfFinalize || op == gq::kPoprfFullEvaluate; }
    bool takes_scalars() const { return op != gq::kTweakClient; }
    bool takes_elems() const { return op == gq::kTweakClient || op == gq::kPoprfFinalize; }
};

int check(const ItemCall &c) {
    const Dims d = dims(c.curve);
    if (!d.ns) return CIRCL_HIP_EPARAM;
    if (c.scalar_stride != 0 && c.scalar_stride != d.ns) return CIRCL_HIP_EPARAM;
    if (c.elem_stride != 0 && c.elem_stride != d.ne) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == gq::kTweakServer && (!c.out2 || !c.out3))) return CIRCL_HIP_EPARAM;
    if (c.takes_scalars() && !c.scalars) return CIRCL_HIP_EPARAM;
    if (c.takes_elems() && !c.elems) return CIRCL_HIP_EPARAM;
    if ((c.input && !c.input_off) || (c.info && !c.info_off)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

constexpr int kItemKernelId[gq::kItemOps] = {CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_FINALIZE,
                                             CIRCL_HIP_KERNEL_OPRF_POPRF_FULL_EVALUATE};

template <class G> int launch_item(const ItemCall &c, const gq::ItemArgs &a, hipStream_t st) {
    const dim3 grid = lanes_grid(c.n), block(64);
    switch (c.op) {
#define DLEQ_ITEM_LAUNCH(OP) case gq::OP: hipLaunchKernelGGL((gq::item_kernel<G, gq::OP>), grid, block, 0, st, a); break
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

// word rows: the scalars and every output but an element row (the tweaked key: out3 of the server's side, out of the client's)
int launch(const ItemCall &c, hipStream_t st) {
    const bool out_words = c.op != gq::kTweakClient;
    if (!aligned<4>(c.scalars, c.out2) || (out_words && !aligned<4>(c.out)) || !aligned<8>(c.input_off, c.info_off)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    gq::ItemArgs a = {};
    a.input = c.takes_input() ? c.input : nullptr;
    a.input_off = a.input ? c.input_off : nullptr;
    a.info = c.info;
    a.info_off = a.info ? c.info_off : nullptr;
    a.scalars = w(c.scalars);
    a.scalar_stride = c.scalar_stride / 4;
    a.elems = c.elems;
    a.elem_stride = c.elem_stride;
    a.out = c.out;
    a.out2 = c.out2;
    a.out3 = c.out3;
    a.ok = c.ok;
    a.n = c.n;
    ProfScope ps(kItemKernelId[c.op], st);
    return c.curve == CIRCL_HIP_P256 ? launch_item<P256>(c, a, st) : launch_item<P384>(c, a, st);
}

int host_pipeline(const ItemCall &c, int device) {
    const Dims d = dims(c.curve);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const bool words_out = c.op != gq::kTweakClient;
    const size_t out_row = c.takes_input() ? d.nh : words_out ? d.ns : d.ne;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<ItemCall> b(c, lo);
        b.rows(&ItemCall::scalars, d.ns, true, c.scalar_stride == 0, c.takes_scalars());
        b.rows(&ItemCall::elems, d.ne, false, c.op == gq::kTweakClient && c.elem_stride == 0, c.takes_elems());
        b.blob(&ItemCall::input, &ItemCall::input_off, true, 0, c.takes_input());   // the client's private input
        b.blob(&ItemCall::info, &ItemCall::info_off, false);
        b.out(&ItemCall::out, out_row, words_out);
        b.out(&ItemCall::out2, d.ns, true, c.op == gq::kTweakServer);
        b.out(&ItemCall::out3, d.ne, false, c.op == gq::kTweakServer);
        b.out(&ItemCall::ok, 1, false);
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

// sk given: the server's side (t, t^-1, t G); pkS given: the client's (the tweaked key only); both or neither: no call
int run_tweak(ItemCall &c, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, bool dev, int device, void *stream) {
    if ((sk != nullptr) == (pkS != nullptr)) return CIRCL_HIP_EPARAM;
    c.op = sk ? gq::kTweakServer : gq::kTweakClient;
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

size_t circl_hip_nistp_dleq_workspace_size(int curve, size_t n_req, size_t n_elems) {
    const Dims d = dims(curve);
    return d.ns ? ws_size(d, n_req, n_elems) : 0;
}

#define DLEQ_FILL(VERIFY)                                                                                                                  \
    Call c;                                                                                                                                \
    c.curve = curve; c.verify = VERIFY; c.kA = kA; c.kA_stride = kA_stride; c.B = B; c.kB = kB; c.off = req_off; c.dst = dst;               \
    c.dst_len = dst_len; c.flags = flags; c.ok = ok; c.n_req = n_req;

int circl_hip_nistp_dleq_prove(int curve, const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req,
                               int device) {
    DLEQ_FILL(false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    return run(c, false, device, nullptr);
}
int circl_hip_nistp_dleq_prove_dev(int curve, const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req,
                                   size_t n_elems, void *d_workspace, size_t workspace_bytes, void *stream) {
    DLEQ_FILL(false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}
int circl_hip_nistp_dleq_verify(int curve, DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, int device) {
    DLEQ_FILL(true)
    c.proofs = const_cast<uint8_t *>(proofs);
    return run(c, false, device, nullptr);
}
int circl_hip_nistp_dleq_verify_dev(int curve, DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, size_t n_elems, void *d_workspace,
                                    size_t workspace_bytes, void *stream) {
    DLEQ_FILL(true)
    c.proofs = const_cast<uint8_t *>(proofs);
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}

BOTH_FORMS(circl_hip_oprf_nistp_poprf_tweak,
           P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob, const uint64_t *info_off,
             uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok),
           {
               ItemCall c;
               c.curve = curve; c.info = info_blob; c.info_off = info_off; c.out = t; c.out2 = t_inv; c.out3 = tweaked; c.ok = ok; c.n = n;
               return run_tweak(c, sk, sk_stride, pkS, pk_stride, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_nistp_poprf_finalize,
           P(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off, const uint8_t *blinds,
             const uint8_t *evaluated, uint8_t *out, uint8_t *ok),
           {
               const Dims d = dims(curve);
               ItemCall c;
               c.curve = curve; c.op = gq::kPoprfFinalize; c.input = input_blob; c.input_off = input_off; c.info = info_blob; c.info_off = info_off;
               c.scalars = blinds; c.scalar_stride = d.ns; c.elems = evaluated; c.elem_stride = d.ne; c.out = out; c.ok = ok; c.n = n;
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_nistp_poprf_full_evaluate,
           P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob,
             const uint64_t *info_off, uint8_t *out, uint8_t *ok),
           {
               ItemCall c;
               c.curve = curve; c.op = gq::kPoprfFullEvaluate; c.scalars = sk; c.scalar_stride = sk_stride; c.input = input_blob; c.input_off = input_off;
               c.info = info_blob; c.info_off = info_off; c.out = out; c.ok = ok; c.n = n;
               return run_call(c, dev_, device, stream);
           })

}  // extern "C"
