// api_nistp.hip -- the batch NIST P-256 / P-384 groups (group/short.go; SEC 1, RFC 9380) and the proof-free part of OPRF (oprf/keys.go,
// oprf/client.go, oprf/server.go; RFC 9497, suites P256-SHA256 and P384-SHA384) behind the C ABI (include/circl_hip.h).  No CPU compute
// path.
//
// The Call, the argument contract, the launch and the host pipeline are oprf_host.h's; here are the entry points and the kernels of the
// two curves.  The curve id is the first thing check() looks at: an unknown one is no group.
#include "oprf_host.h"

using namespace circl::host;
using namespace circl::oprf;

namespace circl {
namespace oprf {
static int launch_group(const Call &c, const Args &a, hipStream_t st) { return c.group == kP256 ? launch_on<P256>(c, a, st) : launch_on<P384>(c, a, st); }
}  // namespace oprf
}  // namespace circl

static Call call_of(int curve, int op, size_t n) {
    Call c;
    c.group = curve == CIRCL_HIP_P256 ? kP256 : curve == CIRCL_HIP_P384 ? kP384 : kNoGroup; c.op = op; c.n = n;
    return c;
}

extern "C" {

BOTH_FORMS(circl_hip_nistp_hash_to_group, P(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *out), {
    Call c = call_of(curve, kHashToGroup, n); c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.flags = flags; c.out = out;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_nistp_hash_to_scalar, P(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c = call_of(curve, kHashToScalar, n); c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_nistp_scalar_mult, P(int curve, const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok), {
    Call c = call_of(curve, kScalarMult, n); c.scalars = scalars; c.scalar_stride = scalar_stride; c.elems = elems; c.flags = flags; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_derive_keypair, P(int curve, int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok), {
    Call c = call_of(curve, kDeriveKeyPair, n); c.mode = mode; c.seeds = seeds; c.blob = info_blob; c.off = info_off; c.out = sk; c.out2 = pk; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_blind, P(int curve, int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok), {
    Call c = call_of(curve, kBlind, n); c.mode = mode; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.out = blinded; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_evaluate, P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok), {
    Call c = call_of(curve, kEvaluate, n); c.scalars = sk; c.scalar_stride = sk_stride; c.elems = blinded; c.out = evaluated; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_finalize, P(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok), {
    Call c = call_of(curve, kFinalize, n); c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.elems = evaluated; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_nistp_full_evaluate, P(int curve, int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok), {
    Call c = call_of(curve, kFullEvaluate, n); c.mode = mode; c.scalars = sk; c.scalar_stride = sk_stride; c.blob = input_blob; c.off = input_off; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

}  // extern "C"
