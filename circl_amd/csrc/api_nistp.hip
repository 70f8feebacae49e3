// api_nistp.hip -- the batch NIST P-256 / P-384 groups (group/short.go; SEC 1, RFC 9380) and the proof-free part of OPRF (oprf/keys.go,
// oprf/client.go, oprf/server.go; RFC 9497, suites P256-SHA256 and P384-SHA384) behind the C ABI (include/circl_hip.h).  No CPU compute
// path.
//
// The shape of api_oprf.hip: every entry point fills one Call (the pointers as the ABI passes them: device pointers for a _dev form, host
// pointers for a host form) and goes through check() -- the argument contract, before any device is looked for -- and then launch() or
// host_pipeline().  Every host form goes through shard / run_pipeline.  Keys, blinds, seeds, the client's inputs and the outputs derived
// from them are flagged secret: their page-locked staging is wiped and the device staging of every chunk is zeroed.  A scalar row that is
// shared by the batch (stride 0: the server's one key) is a per-call input of the pipeline: one row is staged with every chunk.
#include "host_compose.h"
#include "nistp_kernels.h"

using namespace circl::host;
namespace np = circl::nistp;

namespace {

struct Call {
    int curve = CIRCL_HIP_P256, op = np::kHashToGroup, mode = 0;
    const uint8_t *blob = nullptr;       // msg / info / input
    const uint64_t *off = nullptr;
    const uint8_t *dst = nullptr;        // the group-level hashes: the caller's tag (host bytes in both forms)
    size_t dst_len = 0;
    const uint8_t *scalars = nullptr;    // scalars / sk / blinds: rows of Ns
    size_t scalar_stride = 0;
    const uint8_t *elems = nullptr;      // elements / blinded / evaluated: rows of Ne
    const uint8_t *seeds = nullptr;      // rows of 32
    uint32_t flags = 0;
    uint8_t *out = nullptr, *out2 = nullptr, *ok = nullptr;
    size_t n = 0;

    size_t ns() const { return curve == CIRCL_HIP_P256 ? 32 : 48; }   // a scalar; also the suite's hash output
    size_t ne() const { return ns() + 1; }                            // a compressed point
    bool hashes_to_group() const { return op == np::kHashToGroup || op == np::kHashToScalar; }
    bool takes_mode() const { return op == np::kDeriveKeyPair || op == np::kBlind || op == np::kFullEvaluate; }
    bool takes_stride() const { return op == np::kScalarMult || op == np::kEvaluate || op == np::kFullEvaluate; }
    bool takes_blob() const { return op != np::kScalarMult && op != np::kEvaluate; }
    bool takes_scalars() const { return !hashes_to_group() && op != np::kDeriveKeyPair; }
    bool needs_elems() const { return op == np::kEvaluate || op == np::kFinalize; }
    size_t out_row() const { return op == np::kHashToScalar || op == np::kDeriveKeyPair || op == np::kFinalize || op == np::kFullEvaluate ? ns() : ne(); }
};

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (c.curve != CIRCL_HIP_P256 && c.curve != CIRCL_HIP_P384) return CIRCL_HIP_EPARAM;
    if (c.hashes_to_group() && (!c.dst || c.dst_len < 1 || c.dst_len > 255)) return CIRCL_HIP_EPARAM;
    if (c.takes_mode() && (c.mode < 0 || c.mode > (c.op == np::kFullEvaluate ? 1 : 2))) return CIRCL_HIP_EPARAM;
    if (c.takes_stride() && c.scalar_stride != 0 && c.scalar_stride != c.ns()) return CIRCL_HIP_EPARAM;
    if (c.flags & ~1u) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.out || (c.op == np::kDeriveKeyPair && (!c.out2 || !c.seeds))) return CIRCL_HIP_EPARAM;
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
    const char *label = c.op == np::kDeriveKeyPair ? "DeriveKeyPair" : "HashToGroup-";
    const char *ctx_tail = c.curve == CIRCL_HIP_P256 ? "-P256-SHA256" : "-P384-SHA384";
    size_t at = 0;
    auto put = [&](const char *s) { for (; *s; s++) dst[at++] = (uint8_t)*s; };
    put(label);
    put("OPRFV1-");
    dst[at++] = (uint8_t)c.mode;
    put(ctx_tail);
    return at;
}

constexpr int kKernelId[np::kOps] = {CIRCL_HIP_KERNEL_OPRF_HASH_TO_GROUP, CIRCL_HIP_KERNEL_OPRF_HASH_TO_SCALAR, CIRCL_HIP_KERNEL_OPRF_SCALAR_MULT,
                                     CIRCL_HIP_KERNEL_OPRF_DERIVE_KEYPAIR, CIRCL_HIP_KERNEL_OPRF_BLIND, CIRCL_HIP_KERNEL_OPRF_EVALUATE,
                                     CIRCL_HIP_KERNEL_OPRF_FINALIZE, CIRCL_HIP_KERNEL_OPRF_FULL_EVALUATE};

template <class C>
int launch_on(const Call &c, const np::Args &a, hipStream_t st) {
    const dim3 grid = lanes_grid(c.n), block(64);
    switch (c.op) {
#define NISTP_LAUNCH(OP) case np::OP: hipLaunchKernelGGL((np::kernel<C, np::OP>), grid, block, 0, st, a); break
        NISTP_LAUNCH(kHashToGroup);
        NISTP_LAUNCH(kHashToScalar);
        NISTP_LAUNCH(kScalarMult);
        NISTP_LAUNCH(kDeriveKeyPair);
        NISTP_LAUNCH(kBlind);
        NISTP_LAUNCH(kEvaluate);
        NISTP_LAUNCH(kFinalize);
        NISTP_LAUNCH(kFullEvaluate);
#undef NISTP_LAUNCH
        default: return CIRCL_HIP_EPARAM;
    }
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// one launch on device pointers.  Rows of words (scalars, seeds, scalar and hash outputs) are 4-byte aligned; element rows are read and
// written bytewise and need no alignment.
int launch(const Call &c, hipStream_t st) {
    const bool word_out = c.out_row() == c.ns();
    if (!aligned<4>(c.scalars, c.seeds) || (word_out && !aligned<4>(c.out)) || !aligned<8>(c.off)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    np::Args a = {};
    a.blob = c.takes_blob() ? c.blob : nullptr;
    a.off = a.blob ? c.off : nullptr;
    a.scalars = reinterpret_cast<const uint32_t *>(c.scalars);
    a.scalar_stride = c.scalar_stride / 4;
    a.elems = c.elems;
    a.seeds = reinterpret_cast<const uint32_t *>(c.seeds);
    a.out = c.out;
    a.out2 = c.out2;
    a.ok = c.ok;
    a.flags = c.flags;
    a.dst_len = (uint32_t)fill_dst(a.dst, c);
    a.n = c.n;
    ProfScope ps(kKernelId[c.op], st);
    return c.curve == CIRCL_HIP_P256 ? launch_on<np::P256>(c, a, st) : launch_on<np::P384>(c, a, st);
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const bool shared = c.takes_scalars() && c.scalar_stride == 0;
    const bool secret_blob = c.op == np::kBlind || c.op == np::kFinalize || c.op == np::kFullEvaluate;   // the client's private input
    const bool secret_out = c.op == np::kDeriveKeyPair || c.op == np::kFinalize || c.op == np::kFullEvaluate || c.op == np::kScalarMult;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        b.rows(&Call::scalars, c.ns(), true, shared, c.takes_scalars());
        b.rows(&Call::elems, c.ne(), false, false, c.needs_elems() || c.op == np::kScalarMult);
        b.rows(&Call::seeds, 32, true, false, c.op == np::kDeriveKeyPair);
        b.blob(&Call::blob, &Call::off, secret_blob, 0, c.takes_blob());
        b.out(&Call::out, c.out_row(), secret_out);
        b.out(&Call::out2, c.ne(), false, c.op == np::kDeriveKeyPair);
        b.out(&Call::ok, 1, false, !c.hashes_to_group());
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

}  // namespace

extern "C" {

BOTH_FORMS(circl_hip_nistp_hash_to_group, P(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *out), {
    Call c;
    c.curve = curve; c.op = np::kHashToGroup; c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.flags = flags; c.out = out; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_nistp_hash_to_scalar, P(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c;
    c.curve = curve; c.op = np::kHashToScalar; c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_nistp_scalar_mult, P(int curve, const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kScalarMult; c.scalars = scalars; c.scalar_stride = scalar_stride; c.elems = elems; c.flags = flags; c.out = out; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_derive_keypair, P(int curve, int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kDeriveKeyPair; c.mode = mode; c.seeds = seeds; c.blob = info_blob; c.off = info_off; c.out = sk; c.out2 = pk; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_blind, P(int curve, int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kBlind; c.mode = mode; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.out = blinded; c.ok = ok; c.n = n;
    c.scalar_stride = c.ns();
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_evaluate, P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kEvaluate; c.scalars = sk; c.scalar_stride = sk_stride; c.elems = blinded; c.out = evaluated; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_finalize, P(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kFinalize; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.elems = evaluated; c.out = out; c.ok = ok; c.n = n;
    c.scalar_stride = c.ns();
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_full_evaluate, P(int curve, int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok), {
    Call c;
    c.curve = curve; c.op = np::kFullEvaluate; c.mode = mode; c.scalars = sk; c.scalar_stride = sk_stride; c.blob = input_blob; c.off = input_off; c.out = out; c.ok = ok; c.n = n;
    return run_call(c, dev_, device, stream);
})

}  // extern "C"
