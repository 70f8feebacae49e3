// oprf_host.h -- the host layer of the group / base-mode OPRF entry points (api_oprf.hip: ristretto255; api_nistp.hip: P-256, P-384), once.
//
// Every entry point fills one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a host
// form) and goes through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// Every host form goes through shard / run_pipeline.  Keys, blinds, seeds, the client's inputs and the outputs derived from them are
// flagged secret: their page-locked staging is wiped and the device staging of every chunk is zeroed.  A scalar row that is shared
// by the batch (stride 0: the server's one key) is a per-call input of the pipeline: one row is staged with every chunk, never n copies.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
//
// What differs by group is a row of kSuites, read off the group description of oprf_group_kernels.h.  A unit instantiates the kernels of
// its own groups only: it defines launch_group().
#pragma once
#include "host_compose.h"
#include "oprf_group_kernels.h"

namespace circl {
namespace oprf {

struct Call {
    int group = kNoGroup, op = kHashToGroup, mode = 0;
    const uint8_t *blob = nullptr;       // msg / info / input
    const uint64_t *off = nullptr;
    const uint8_t *dst = nullptr;        // the group-level hashes: the caller's tag (host bytes in both forms)
    size_t dst_len = 0;
    const uint8_t *scalars = nullptr;    // scalars / sk / blinds: rows of ns
    size_t scalar_stride = 0;            // where the operation takes one (takes_stride); otherwise the rows are packed
    const uint8_t *elems = nullptr;      // elements / blinded / evaluated: rows of ne
    const uint8_t *seeds = nullptr;      // rows of 32
    uint32_t flags = 0;
    uint8_t *out = nullptr, *out2 = nullptr, *ok = nullptr;
    size_t n = 0;

    const Suite &suite() const { return kSuites[group]; }
    bool hashes_to_group() const { return op == kHashToGroup || op == kHashToScalar; }
    bool takes_mode() const { return op == kDeriveKeyPair || op == kBlind || op == kFullEvaluate; }
    bool takes_stride() const { return op == kScalarMult || op == kEvaluate || op == kFullEvaluate; }
    bool takes_blob() const { return op != kScalarMult && op != kEvaluate; }
    bool takes_scalars() const { return !hashes_to_group() && op != kDeriveKeyPair; }
    bool needs_elems() const { return op == kEvaluate || op == kFinalize; }
    bool writes_elems() const { return op == kHashToGroup || op == kScalarMult || op == kBlind || op == kEvaluate; }
    size_t stride() const { return takes_stride() ? scalar_stride : suite().ns; }
    size_t out_row() const { return writes_elems() ? suite().ne : op == kFinalize || op == kFullEvaluate ? suite().nh : suite().ns; }
};

// the argument contract, the same for both forms; nothing here looks for a device
static int check(const Call &c) {
    if (c.group < 0 || c.group >= kGroups) return CIRCL_HIP_EPARAM;
    if (c.hashes_to_group() && (!c.dst || c.dst_len < 1 || c.dst_len > 255)) return CIRCL_HIP_EPARAM;
    if (c.takes_mode() && (c.mode < 0 || c.mode > (c.op == kFullEvaluate ? 1 : 2))) return CIRCL_HIP_EPARAM;
    if (c.takes_stride() && c.scalar_stride != 0 && c.scalar_stride != c.suite().ns) return CIRCL_HIP_EPARAM;
    if (c.flags & ~1u) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == kDeriveKeyPair && (!c.out2 || !c.seeds))) return CIRCL_HIP_EPARAM;
    if (c.takes_scalars() && !c.scalars) return CIRCL_HIP_EPARAM;
    if (c.needs_elems() && !c.elems) return CIRCL_HIP_EPARAM;
    if (c.takes_blob() && c.blob && !c.off) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

// the tag of a launch's expand_message_xmd: the caller's, or the label of the operation and the suite's context string
static size_t fill_dst(uint8_t (&dst)[256], const Call &c) {
    if (c.hashes_to_group()) {
        memcpy(dst, c.dst, c.dst_len);
        return c.dst_len;
    }
    size_t at = 0;
    auto put = [&](const char *s) { for (; *s; s++) dst[at++] = (uint8_t)*s; };
    put(c.op == kDeriveKeyPair ? "DeriveKeyPair" : "HashToGroup-");
    put("OPRFV1-");
    dst[at++] = (uint8_t)c.mode;
    put(c.suite().ctx_tail);
    return at;
}

constexpr int kKernelId[kOps] = {CIRCL_HIP_KERNEL_OPRF_HASH_TO_GROUP, CIRCL_HIP_KERNEL_OPRF_HASH_TO_SCALAR, CIRCL_HIP_KERNEL_OPRF_SCALAR_MULT,
                                 CIRCL_HIP_KERNEL_OPRF_DERIVE_KEYPAIR, CIRCL_HIP_KERNEL_OPRF_BLIND, CIRCL_HIP_KERNEL_OPRF_EVALUATE,
                                 CIRCL_HIP_KERNEL_OPRF_FINALIZE, CIRCL_HIP_KERNEL_OPRF_FULL_EVALUATE};

// the kernel of c.op for group G
template <class G> static int launch_on(const Call &c, const Args &a, hipStream_t st) {
    const dim3 grid = host::lanes_grid(c.n), block(64);
    switch (c.op) {
#define OPRF_LAUNCH(OP) case OP: hipLaunchKernelGGL((kernel<G, OP>), grid, block, 0, st, a); break
        OPRF_LAUNCH(kHashToGroup);
        OPRF_LAUNCH(kHashToScalar);
        OPRF_LAUNCH(kScalarMult);
        OPRF_LAUNCH(kDeriveKeyPair);
        OPRF_LAUNCH(kBlind);
        OPRF_LAUNCH(kEvaluate);
        OPRF_LAUNCH(kFinalize);
        OPRF_LAUNCH(kFullEvaluate);
#undef OPRF_LAUNCH
        default: return CIRCL_HIP_EPARAM;
    }
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}
// the unit's own: launch_on<G> for the group of c among the groups the unit serves
static int launch_group(const Call &c, const Args &a, hipStream_t st);

// one launch on device pointers.  Rows of words (scalars, seeds, scalar and hash outputs) are 4-byte aligned; element rows as their
// group reads them: words (ristretto255) or bytes (the NIST curves: no alignment).
static int launch(const Call &c, hipStream_t st) {
    const size_t ea = c.suite().elem_align;
    auto elem_aligned = [&](const uint8_t *p) { return reinterpret_cast<uintptr_t>(p) % ea == 0; };
    const bool words_ok = host::aligned<4>(c.scalars, c.seeds) && host::aligned<8>(c.off);
    const bool elems_ok = elem_aligned(c.elems) && elem_aligned(c.out2);                                       // out2: the public keys
    const bool out_ok = c.writes_elems() ? elem_aligned(c.out) : host::aligned<4>(c.out);                      // element rows, or word rows
    if (!words_ok || !elems_ok || !out_ok) return CIRCL_HIP_EWORKSPACE;
    if (host::ndev() <= 0) return CIRCL_HIP_ENODEV;
    Args a = {};
    a.blob = c.takes_blob() ? c.blob : nullptr;
    a.off = a.blob ? c.off : nullptr;
    a.scalars = reinterpret_cast<const uint32_t *>(c.scalars);
    a.scalar_stride = c.stride() / 4;
    a.elems = c.elems;
    a.seeds = reinterpret_cast<const uint32_t *>(c.seeds);
    a.out = c.out;
    a.out2 = c.out2;
    a.ok = c.ok;
    a.flags = c.flags;
    a.dst_len = (uint32_t)fill_dst(a.dst, c);
    a.n = c.n;
    host::ProfScope ps(kKernelId[c.op], st);
    return launch_group(c, a, st);
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
static int host_pipeline(const Call &c, int device) {
    using namespace host;
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const Suite &s = c.suite();
    const bool shared = c.takes_scalars() && c.stride() == 0;
    const bool secret_blob = c.op == kBlind || c.op == kFinalize || c.op == kFullEvaluate;   // the client's private input
    const bool secret_out = c.op == kDeriveKeyPair || c.op == kFinalize || c.op == kFullEvaluate || c.op == kScalarMult;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        b.rows(&Call::scalars, s.ns, true, shared, c.takes_scalars());
        b.rows(&Call::elems, s.ne, false, false, c.needs_elems() || c.op == kScalarMult);
        b.rows(&Call::seeds, 32, true, false, c.op == kDeriveKeyPair);
        b.blob(&Call::blob, &Call::off, secret_blob, 0, c.takes_blob());
        b.out(&Call::out, c.out_row(), secret_out);
        b.out(&Call::out2, s.ne, false, c.op == kDeriveKeyPair);
        b.out(&Call::ok, 1, false, !c.hashes_to_group());
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

}  // namespace oprf
}  // namespace circl
