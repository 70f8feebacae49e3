// dleq_host.h -- the host layer of the DLEQ proof and mode-2 (POPRF) entry points (api_dleq.hip: ristretto255; api_dleq_nistp.hip: P-256,
// P-384), once.
//
// As in oprf_host.h every entry point fills one Call and goes through check() -- the argument contract, before any device is looked
// for -- and then launch() or host_pipeline().  The proofs' item is the REQUEST: the pipeline and shard split on requests, the element
// arrays travel as blobs over ONE scaled copy of req_off (x Ne bytes) that is built once per call, and a launch gets the chunk's
// offsets in bytes with the divisor Ne (gdleq::Args::off_div).  k and r are secret: their staging is wiped and the device staging of
// every chunk is zeroed, except the workspace, which holds sums of public points only.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
//
// What differs by group is a row of oprf::kSuites and the words of a point in the workspace (kPointWords).  A unit instantiates the
// kernels of its own groups only: it defines the two launch_group().
#pragma once
#include "dleq_group_kernels.h"
#include "host_compose.h"

namespace circl {
namespace gdleq {

using namespace host;
using oprf::Suite;

inline const uint32_t *words(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
inline uint32_t *words(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }
inline bool elems_aligned(const Suite &s, std::initializer_list<const uint8_t *> rows) {
    for (const uint8_t *p : rows)
        if (reinterpret_cast<uintptr_t>(p) % s.elem_align) return false;
    return true;
}

constexpr size_t kMaxCtx = 255 - kTagHead;   // "HashToScalar-" || dst must fit xmd's tag
constexpr size_t kPointWords[oprf::kGroups] = {Ops<oprf::R255>::PW, Ops<oprf::P256>::PW, Ops<oprf::P384>::PW};
inline bool is_group(int group) { return group >= 0 && group < oprf::kGroups; }

// ---- the proofs ----------------------------------------------------------------------------------------------------------------
struct Call {
    int group = oprf::kNoGroup;
    bool verify = false;
    const uint8_t *k = nullptr, *kA = nullptr, *B = nullptr, *kB = nullptr, *r = nullptr, *dst = nullptr;
    size_t k_stride = 0, kA_stride = 0, dst_len = 0;
    const uint64_t *off = nullptr;
    uint32_t off_div = 1, flags = 0;
    uint8_t *proofs = nullptr, *ok = nullptr;   // verify reads the proofs
    size_t n_req = 0, n_elems = 0;
    uint8_t *ws = nullptr;
    size_t ws_bytes = 0;

    const Suite &suite() const { return oprf::kSuites[group]; }
};

inline size_t slots(size_t n_req, size_t n_elems) { return (n_elems + 63) / 64 + n_req; }
inline size_t ws_size(int group, size_t n_req, size_t n_elems) { return up256(4 * n_req) + up256(slots(n_req, n_elems) * 2 * kPointWords[group] * 4); }

// the argument contract, the same for both forms; nothing here looks for a device
static int check(const Call &c) {
    if (!is_group(c.group)) return CIRCL_HIP_EPARAM;
    if (c.kA_stride != 0 && c.kA_stride != c.suite().ne) return CIRCL_HIP_EPARAM;
    if (!c.verify && c.k_stride != 0 && c.k_stride != c.suite().ns) return CIRCL_HIP_EPARAM;
    if (c.dst_len > kMaxCtx || (c.dst_len && !c.dst)) return CIRCL_HIP_EPARAM;
    if (c.flags & ~kNoIdentity) return CIRCL_HIP_EPARAM;
    if (c.n_req == 0) return CIRCL_HIP_OK;
    if (!c.kA || !c.B || !c.kB || !c.off || !c.proofs) return CIRCL_HIP_EPARAM;
    if (c.verify ? !c.ok : (!c.k || !c.r)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

// the two kernels of a call for group G
template <class G> static void launch_on(const Call &c, const Args &a, bool finishing, hipStream_t st) {
    const dim3 grid = lanes_grid(finishing ? c.n_req : c.n_elems), block(64);
    if (finishing) {
        if (c.verify) hipLaunchKernelGGL((finish<G, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((finish<G, false>), grid, block, 0, st, a);
    } else {
        if (c.verify) hipLaunchKernelGGL((composite<G, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((composite<G, false>), grid, block, 0, st, a);
    }
}
// the unit's own: launch_on<G> for the group of c among the groups the unit serves
static void launch_group(const Call &c, const Args &a, bool finishing, hipStream_t st);

// two launches on device pointers.  Scalar and proof rows are words; element rows (kA, B, kB) as their group reads them: words
// (ristretto255) or bytes (the NIST curves: no alignment).
static int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.k, c.r, c.proofs) || !elems_aligned(c.suite(), {c.kA, c.B, c.kB}) || !aligned<8>(c.off) || !aligned<8>(c.ws)) return CIRCL_HIP_EWORKSPACE;
    if (!c.ws || c.ws_bytes < ws_size(c.group, c.n_req, c.n_elems)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    Args a = {};
    a.off = c.off;
    a.off_div = c.off_div;
    a.B = c.B;
    a.kB = c.kB;
    a.k = words(c.k);
    a.k_stride = c.k_stride / 4;
    a.kA = c.kA;
    a.kA_stride = c.kA_stride;
    a.r = words(c.r);
    a.proofs = words(c.proofs);
    a.ok = c.ok;
    a.bad = words(c.ws);
    a.partial = words(c.ws + up256(4 * c.n_req));
    a.n_req = c.n_req;
    a.n_elems = c.n_elems;
    a.flags = c.flags;
    memcpy(a.tag, "HashToScalar-", kTagHead);
    if (c.dst_len) memcpy(a.tag + kTagHead, c.dst, c.dst_len);
    a.tag_len = (uint32_t)(kTagHead + c.dst_len);
    HIP_TRY(hipMemsetAsync(a.bad, 0, 4 * c.n_req, st));
    if (c.n_elems) {
        ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_COMPOSITE, st);
        launch_group(c, a, false, st);
        HIP_TRY(hipGetLastError());
    }
    ProfScope ps(CIRCL_HIP_KERNEL_DLEQ_FINISH, st);
    launch_group(c, a, true, st);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host form: shard / run_pipeline over requests --------------------------------------------------------------------------------
static int host_pipeline(const Call &c, int device) {
    const Suite &s = c.suite();
    // the one scaled copy of the offsets: the element arrays are blobs of Ne-byte rows, staged from the call that holds it
    std::vector<uint64_t> scaled(c.n_req + 1);
    for (size_t g = 0; g <= c.n_req; g++) scaled[g] = c.off[g] * s.ne;
    Call sc = c;
    sc.off = scaled.data();
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 14);
    opts.wipe_device = !c.verify;
    opts.ws_secret_bytes = [](size_t) { return size_t(0); };   // partial sums of d_j B_j: public
    return shard(c.n_req, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(sc, lo, &Call::n_req);
        b.rows(&Call::kA, s.ne, false, c.kA_stride == 0);
        b.rows(&Call::k, s.ns, true, c.k_stride == 0, !c.verify);
        b.rows(&Call::r, s.ns, true, false, !c.verify);
        if (c.verify) b.rows(&Call::proofs, 2 * s.ns, false);
        else b.out(&Call::proofs, 2 * s.ns, false);
        b.blob(&Call::B, &Call::off, false);
        b.blob(&Call::kB, &Call::off, false);    // (each blob stages the offsets; a launch reads one copy)
        b.out(&Call::ok, 1, false);
        // a chunk's workspace: sized for the chunk of this shard that has the most elements
        const size_t chunk = std::max<size_t>(1, std::min(cnt, opts.chunk_items));
        size_t most = 0;
        for (size_t from = lo; from < lo + cnt; from += chunk) most = std::max<size_t>(most, c.off[std::min(from + chunk, lo + cnt)] - c.off[from]);
        size_t at = lo;   // the chunks of a shard are launched in order, on this thread
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, [&](size_t n) { return ws_size(c.group, n, most); }, opts, [&](Chunk &k) {
            Call d = b.on(k);
            d.off_div = (uint32_t)s.ne;
            d.n_elems = c.off[at + k.cnt] - c.off[at];
            at += k.cnt;
            d.ws = k.ws;
            d.ws_bytes = k.ws_bytes;
            return launch(d, k.st);
        });
    }, kHeavyOneDeviceMax);
}

static int run(Call &c, bool dev, int device, void *stream) {
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
    int group = oprf::kNoGroup, op = kTweakServer;
    const uint8_t *input = nullptr, *info = nullptr, *scalars = nullptr, *elems = nullptr;
    const uint64_t *input_off = nullptr, *info_off = nullptr;
    size_t scalar_stride = 0, elem_stride = 0;   // where the operation takes one; otherwise the rows are packed
    uint8_t *out = nullptr, *out2 = nullptr, *out3 = nullptr, *ok = nullptr;
    size_t n = 0;

    const Suite &suite() const { return oprf::kSuites[group]; }
    bool takes_input() const { return op == kPoprfFinalize || op == kPoprfFullEvaluate; }
    bool takes_scalars() const { return op != kTweakClient; }
    bool takes_elems() const { return op == kTweakClient || op == kPoprfFinalize; }
    bool writes_elem() const { return op == kTweakClient; }   // out is the tweaked key, an element row; every other out is a row of words
    size_t stride() const { return op == kPoprfFinalize ? suite().ns : scalar_stride; }   // (finalize: the blinds)
    size_t elem_step() const { return op == kTweakClient ? elem_stride : suite().ne; }
    size_t out_row() const { return takes_input() ? suite().nh : writes_elem() ? suite().ne : suite().ns; }
};

static int check(const ItemCall &c) {
    if (!is_group(c.group)) return CIRCL_HIP_EPARAM;
    if (c.scalar_stride != 0 && c.scalar_stride != c.suite().ns) return CIRCL_HIP_EPARAM;
    if (c.elem_stride != 0 && c.elem_stride != c.suite().ne) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == kTweakServer && (!c.out2 || !c.out3))) return CIRCL_HIP_EPARAM;
    if (c.takes_scalars() && !c.scalars) return CIRCL_HIP_EPARAM;
    if (c.takes_elems() && !c.elems) return CIRCL_HIP_EPARAM;
    if ((c.input && !c.input_off) || (c.info && !c.info_off)) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

constexpr int kItemKernelId[kItemOps] = {CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK, CIRCL_HIP_KERNEL_OPRF_POPRF_FINALIZE,
                                         CIRCL_HIP_KERNEL_OPRF_POPRF_FULL_EVALUATE};

// the kernel of c.op for group G
template <class G> static int launch_on(const ItemCall &c, const ItemArgs &a, hipStream_t st) {
    const dim3 grid = lanes_grid(c.n), block(64);
    switch (c.op) {
#define DLEQ_ITEM_LAUNCH(OP) case OP: hipLaunchKernelGGL((item_kernel<G, OP>), grid, block, 0, st, a); break
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
static int launch_group(const ItemCall &c, const ItemArgs &a, hipStream_t st);

// word rows: the scalars and every output but an element row (the tweaked key: out3 of the server's side, out of the client's)
static int launch(const ItemCall &c, hipStream_t st) {
    const bool words_ok = aligned<4>(c.scalars, c.out2) && (c.writes_elem() || aligned<4>(c.out)) && aligned<8>(c.input_off, c.info_off);
    if (!words_ok || !elems_aligned(c.suite(), {c.elems, c.out3, c.writes_elem() ? c.out : nullptr})) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    ItemArgs a = {};
    a.input = c.takes_input() ? c.input : nullptr;
    a.input_off = a.input ? c.input_off : nullptr;
    a.info = c.info;
    a.info_off = a.info ? c.info_off : nullptr;
    a.scalars = words(c.scalars);
    a.scalar_stride = c.stride() / 4;
    a.elems = c.elems;
    a.elem_stride = c.elem_step();
    a.out = c.out;
    a.out2 = c.out2;
    a.out3 = c.out3;
    a.ok = c.ok;
    a.n = c.n;
    ProfScope ps(kItemKernelId[c.op], st);
    return launch_group(c, a, st);
}

static int host_pipeline(const ItemCall &c, int device) {
    const Suite &s = c.suite();
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<ItemCall> b(c, lo);
        b.rows(&ItemCall::scalars, s.ns, true, c.stride() == 0, c.takes_scalars());
        b.rows(&ItemCall::elems, s.ne, false, c.elem_step() == 0, c.takes_elems());
        b.blob(&ItemCall::input, &ItemCall::input_off, true, 0, c.takes_input());   // the client's private input
        b.blob(&ItemCall::info, &ItemCall::info_off, false);
        b.out(&ItemCall::out, c.out_row(), !c.writes_elem());
        b.out(&ItemCall::out2, s.ns, true, c.op == kTweakServer);
        b.out(&ItemCall::out3, s.ne, false, c.op == kTweakServer);
        b.out(&ItemCall::ok, 1, false);
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

// sk given: the server's side (t, t^-1, t G); pkS given: the client's (the tweaked key only); both or neither: no call
static int run_tweak(ItemCall &c, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, bool dev, int device, void *stream) {
    if ((sk != nullptr) == (pkS != nullptr)) return CIRCL_HIP_EPARAM;
    c.op = sk ? kTweakServer : kTweakClient;
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

}  // namespace gdleq
}  // namespace circl

// ---- what the entry points of both units share: NAME(..., DLEQ_PARAMS_, ..., DLEQ_TAIL_, ...) and the Call they fill ------------------
#define DLEQ_PARAMS_ const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off
#define DLEQ_TAIL_ const uint8_t *dst, size_t dst_len, uint32_t flags
#define DLEQ_FILL(GROUP, VERIFY)                                                                                                           \
    circl::gdleq::Call c;                                                                                                                   \
    c.group = GROUP; c.verify = VERIFY; c.kA = kA; c.kA_stride = kA_stride; c.B = B; c.kB = kB; c.off = req_off; c.dst = dst;               \
    c.dst_len = dst_len; c.flags = flags; c.ok = ok; c.n_req = n_req;
