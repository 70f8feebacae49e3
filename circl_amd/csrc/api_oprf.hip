// api_oprf.hip -- the batch ristretto255 group (group/ristretto255.go; RFC 9496, RFC 9380) and the proof-free part of OPRF (oprf/keys.go,
// oprf/client.go, oprf/server.go; RFC 9497, suite ristretto255-SHA512) behind the C ABI (include/circl_hip.h).  No CPU compute path.
//
// The Call, the argument contract, the launch and the host pipeline are oprf_host.h's; here are the entry points and the ristretto255
// kernels.
#include "oprf_host.h"

using namespace circl::host;
using namespace circl::oprf;

namespace circl {
namespace oprf {
static int launch_group(const Call &c, const Args &a, hipStream_t st) { return launch_on<R255>(c, a, st); }
}  // namespace oprf
}  // namespace circl

static Call call_of(int op, size_t n) {
    Call c;
    c.group = kR255; c.op = op; c.n = n;
    return c;
}

extern "C" {

BOTH_FORMS(circl_hip_ristretto255_hash_to_group, P(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c = call_of(kHashToGroup, n); c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_ristretto255_hash_to_scalar, P(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out), {
    Call c = call_of(kHashToScalar, n); c.blob = msg_blob; c.off = msg_off; c.dst = dst; c.dst_len = dst_len; c.out = out;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_ristretto255_scalar_mult, P(const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok), {
    Call c = call_of(kScalarMult, n); c.scalars = scalars; c.scalar_stride = scalar_stride; c.elems = elems; c.flags = flags; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_derive_keypair, P(int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok), {
    Call c = call_of(kDeriveKeyPair, n); c.mode = mode; c.seeds = seeds; c.blob = info_blob; c.off = info_off; c.out = sk; c.out2 = pk; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_blind, P(int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok), {
    Call c = call_of(kBlind, n); c.mode = mode; c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.out = blinded; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_evaluate, P(const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok), {
    Call c = call_of(kEvaluate, n); c.scalars = sk; c.scalar_stride = sk_stride; c.elems = blinded; c.out = evaluated; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_finalize, P(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok), {
    Call c = call_of(kFinalize, n); c.blob = input_blob; c.off = input_off; c.scalars = blinds; c.elems = evaluated; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_oprf_full_evaluate, P(int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok), {
    Call c = call_of(kFullEvaluate, n); c.mode = mode; c.scalars = sk; c.scalar_stride = sk_stride; c.blob = input_blob; c.off = input_off; c.out = out; c.ok = ok;
    return run_call(c, dev_, device, stream);
})

}  // extern "C"
