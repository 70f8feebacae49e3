// api_oprf.hip -- the batch ristretto255 group (group/ristretto255.go; RFC 9496, RFC 9380) and the proof-free part of OPRF (oprf/keys.go,
// oprf/client.go, oprf/server.go; RFC 9497, suite ristretto255-SHA512) behind the C ABI (include/circl_hip.h).  No CPU compute path.
//
// Every entry point fills one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a host
// form) and goes through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// Every host form goes through shard / run_pipeline.  Keys, blinds, seeds, the client's inputs and the outputs derived from them are
// flagged secret: their page-locked staging is wiped and the device staging of every chunk is zeroed.  A scalar row that is shared
// by the batch (stride 0: the server's one key) is a per-call input of the pipeline: one row is staged with every chunk, never n copies.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
#include "host_compose.h"
#include "oprf_kernels.h"

using namespace circl::host;
namespace op = circl::oprf;

namespace {

struct Call {
    int op = op::kHashToGroup, mode = 0;
    const uint8_t *blob = nullptr;       // msg / info / input
    const uint64_t *off = nullptr;
    const uint8_t *dst = nullptr;        // the group-level hashes: the caller's tag (host bytes in both forms)
    size_t dst_len = 0;
    const uint8_t *scalars = nullptr;    // scalars / sk / blinds
    size_t scalar_stride = 32;
    const uint8_t *elems = nullptr;      // elements / seeds / blinded / evaluated
    uint32_t flags = 0;
    uint8_t *out = nullptr, *out2 = nullptr, *ok = nullptr;
    size_t n = 0;

    bool hashes_to_group() const { return op == op::kHashToGroup || op == op::kHashToScalar; }
    bool takes_mode() const { return op == op::kDeriveKeyPair || op == op::kBlind || op == op::kFullEvaluate; }
    bool takes_stride() const { return op == op::kScalarMult || op == op::kEvaluate || op == op::kFullEvaluate; }
    bool takes_blob() const { return op != op::kScalarMult && op != op::kEvaluate; }
    bool takes_scalars() const { return !hashes_to_group() && op != op::kDeriveKeyPair; }
    bool needs_elems() const { return op == op::kDeriveKeyPair || op == op::kEvaluate || op == op::kFinalize; }
    size_t out_row() const { return op == op::kFinalize || op == op::kFullEvaluate ? 64 : 32; }
};

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (c.hashes_to_group() && (!c.dst || c.dst_len < 1 || c.dst_len > 255)) return CIRCL_HIP_EPARAM;
    if (c.takes_mode() && (c.mode < 0 || c.mode > (c.op == op::kFullEvaluate ? 1 : 2))) return CIRCL_HIP_EPARAM;
    if (c.takes_stride() && c.scalar_stride != 0 && c.scalar_stride != 32) return CIRCL_HIP_EPARAM;
    if (c.flags & ~1u) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == op::kDeriveKeyPair && !c.out2)) return CIRCL_HIP_EPARAM;
    if (c.takes_scalars() && !c.scalars) return CIRCL_HIP_EPARAM;
    if (c.needs_elems() && !c.elems) return CIRCL_HIP_EPARAM;
    if (c.takes_blob() && c.blob && !c.off) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

// the tag of a launch's expand_message_xmd: the caller's, or the label of the operation and the suite's context string
size_t fill_dst(uint8_t (&dst)[256], const Call &c) {
    if (c.hashes_to_group()) {
        memcpy(dst, c.dst, c.dst_len);
        return c.dst_len;
    }
    const char *label = c.op == op::kDeriveKeyPair ? "DeriveKeyPair" : "HashToGroup-";
    const char ctx_head[] = "OPRFV1-", ctx_tail[] = "-ristretto255-SHA512";
    size_t at = 0;
    auto put = [&](const char *s) { for (; *s; s++) dst[at++] = (uint8_t)*s; };
    put(label);
    put(ctx_head);
    dst[at++] = (uint8_t)c.mode;
    put(ctx_tail);
    return at;
}

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *w(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

constexpr int kKernelId[op::kOps] = {CIRCL_HIP_KERNEL_OPRF_HASH_TO_GROUP, CIRCL_HIP_KERNEL_OPRF_HASH_TO_SCALAR, CIRCL_HIP_KERNEL_OPRF_SCALAR_MULT,
                                     CIRCL_HIP_KERNEL_OPRF_DERIVE_KEYPAIR, CIRCL_HIP_KERNEL_OPRF_BLIND, CIRCL_HIP_KERNEL_OPRF_EVALUATE,
                                     CIRCL_HIP_KERNEL_OPRF_FINALIZE, CIRCL_HIP_KERNEL_OPRF_FULL_EVALUATE};

// one launch on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.scalars, c.elems, c.out, c.out2) || !aligned<8>(c.off)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    op::Args a = {};
    a.blob = c.takes_blob() ? c.blob : nullptr;
    a.off = a.blob ? c.off : nullptr;
    a.scalars = w(c.scalars);
    a.scalar_stride = c.scalar_stride / 4;
    a.elems = w(c.elems);
    a.out = w(c.out);
    a.out2 = w(c.out2);
    a.ok = c.ok;
    a.flags = c.flags;
    a.dst_len = (uint32_t)fill_dst(a.dst, c);
    a.n = c.n;
    const dim3 grid = lanes_grid(c.n), block(64);
    ProfScope ps(kKernelId[c.op], st);
    switch (c.op) {
#define OPRF_LAUNCH(OP) case op::OP: hipLaunchKernelGGL(op::kernel<op::OP>, grid, block, 0, st, a); break
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

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const bool shared = c.takes_scalars() && c.scalar_stride == 0;
    const bool secret_blob = c.op == op::kBlind || c.op == op::kFinalize || c.op == op::kFullEvaluate;   // the client's private input
    const bool secret_elems = c.op == op::kDeriveKeyPair;                                               // seeds
    const bool secret_out = c.op == op::kDeriveKeyPair || c.op == op::kFinalize || c.op == op::kFullEvaluate || c.op == op::kScalarMult;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        b.rows(&Call::scalars, 32, true, shared, c.takes_scalars());
        b.rows(&Call::elems, 32, secret_elems, false, c.needs_elems() || c.op == op::kScalarMult);
        b.blob(&Call::blob, &Call::off, secret_blob, 0, c.takes_blob());
        b.out(&Call::out, c.out_row(), secret_out);
        b.out(&Call::out2, 32, false, c.op == op::kDeriveKeyPair);
        b.out(&Call::ok, 1, false, !c.hashes_to_group());
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

}  // namespace

extern "C" {

BOTH_FORMS(circl_hip_ristretto255_hash_to_group, P(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c;
    c.op = op::kHashToGroup; c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_ristretto255_hash_to_scalar, P(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c;
    c.op = op::kHashToScalar; c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_ristretto255_scalar_mult, P(const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok), {
    Call c;
    c.op = op::kScalarMult; c.scalars = scalars; c.scalar_stride = scalar_stride; c.elems = elems; c.flags = flags; c.out = out; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_derive_keypair, P(int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok), {
    Call c;
    c.op = op::kDeriveKeyPair; c.mode = mode; c.elems = seeds; c.blob = info_blob; c.off = info_off; c.out = sk; c.out2 = pk; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_blind, P(int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok), {
    Call c;
    c.op = op::kBlind; c.mode = mode; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.out = blinded; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_evaluate, P(const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok), {
    Call c;
    c.op = op::kEvaluate; c.scalars = sk; c.scalar_stride = sk_stride; c.elems = blinded; c.out = evaluated; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_finalize, P(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok), {
    Call c;
    c.op = op::kFinalize; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.elems = evaluated; c.out = out; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_full_evaluate, P(int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok), {
    Call c;
    c.op = op::kFullEvaluate; c.mode = mode; c.scalars = sk; c.scalar_stride = sk_stride; c.blob = input_blob; c.off = input_off; c.out = out; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

}  // extern "C"
