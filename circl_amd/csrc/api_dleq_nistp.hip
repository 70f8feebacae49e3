// api_dleq_nistp.hip -- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms; RFC 9497 section 2.2) on P-256 and P-384 and the mode-2
// (POPRF) item operations of oprf/client.go and oprf/server.go for suites P256-SHA256 and P384-SHA384, behind the C ABI
// (include/circl_hip.h).  No CPU compute path.  The kernels are dleq_group_kernels.h's, instantiated for the two curves here and
// nowhere else: the NIST field code is expensive to compile, and a unit of its own keeps that off the other units' build.
//
// The Calls, the argument contract, the launches and the host pipelines are dleq_host.h's; here are the entry points and the kernels of
// the two curves.  The curve id is the first thing check() looks at: an unknown one is no group.
#include "dleq_host.h"

using namespace circl::host;
using namespace circl::gdleq;
using circl::oprf::kP256;
using circl::oprf::P256;
using circl::oprf::P384;

namespace circl {
namespace gdleq {
static void launch_group(const Call &c, const Args &a, bool finishing, hipStream_t st) {
    if (c.group == kP256) launch_on<P256>(c, a, finishing, st);
    else launch_on<P384>(c, a, finishing, st);
}
static int launch_group(const ItemCall &c, const ItemArgs &a, hipStream_t st) { return c.group == kP256 ? launch_on<P256>(c, a, st) : launch_on<P384>(c, a, st); }
}  // namespace gdleq
}  // namespace circl

static int group_of(int curve) { return curve == CIRCL_HIP_P256 ? kP256 : curve == CIRCL_HIP_P384 ? circl::oprf::kP384 : circl::oprf::kNoGroup; }

static ItemCall item_of(int curve, int op, size_t n) {
    ItemCall c;
    c.group = group_of(curve); c.op = op; c.n = n;
    return c;
}

extern "C" {

size_t circl_hip_nistp_dleq_workspace_size(int curve, size_t n_req, size_t n_elems) {
    return is_group(group_of(curve)) ? ws_size(group_of(curve), n_req, n_elems) : 0;
}

int circl_hip_nistp_dleq_prove(int curve, const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req,
                               int device) {
    DLEQ_FILL(group_of(curve), false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    return run(c, false, device, nullptr);
}
int circl_hip_nistp_dleq_prove_dev(int curve, const uint8_t *k, size_t k_stride, DLEQ_PARAMS_, const uint8_t *r, DLEQ_TAIL_, uint8_t *proofs, uint8_t *ok, size_t n_req,
                                   size_t n_elems, void *d_workspace, size_t workspace_bytes, void *stream) {
    DLEQ_FILL(group_of(curve), false)
    c.k = k; c.k_stride = k_stride; c.r = r; c.proofs = proofs;
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}
int circl_hip_nistp_dleq_verify(int curve, DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, int device) {
    DLEQ_FILL(group_of(curve), true)
    c.proofs = const_cast<uint8_t *>(proofs);
    return run(c, false, device, nullptr);
}
int circl_hip_nistp_dleq_verify_dev(int curve, DLEQ_PARAMS_, const uint8_t *proofs, DLEQ_TAIL_, uint8_t *ok, size_t n_req, size_t n_elems, void *d_workspace,
                                    size_t workspace_bytes, void *stream) {
    DLEQ_FILL(group_of(curve), true)
    c.proofs = const_cast<uint8_t *>(proofs);
    c.n_elems = n_elems; c.ws = static_cast<uint8_t *>(d_workspace); c.ws_bytes = workspace_bytes;
    return run(c, true, 0, stream);
}

BOTH_FORMS(circl_hip_oprf_nistp_poprf_tweak,
           P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob, const uint64_t *info_off,
             uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok),
           {
               ItemCall c = item_of(curve, kTweakServer, n);
               c.info = info_blob; c.info_off = info_off; c.out = t; c.out2 = t_inv; c.out3 = tweaked; c.ok = ok;
               return run_tweak(c, sk, sk_stride, pkS, pk_stride, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_nistp_poprf_finalize,
           P(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off, const uint8_t *blinds,
             const uint8_t *evaluated, uint8_t *out, uint8_t *ok),
           {
               ItemCall c = item_of(curve, kPoprfFinalize, n);
               c.input = input_blob; c.input_off = input_off; c.info = info_blob; c.info_off = info_off; c.scalars = blinds; c.elems = evaluated;
               c.out = out; c.ok = ok;
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_oprf_nistp_poprf_full_evaluate,
           P(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob,
             const uint64_t *info_off, uint8_t *out, uint8_t *ok),
           {
               ItemCall c = item_of(curve, kPoprfFullEvaluate, n);
               c.scalars = sk; c.scalar_stride = sk_stride; c.input = input_blob; c.input_off = input_off; c.info = info_blob; c.info_off = info_off;
               c.out = out; c.ok = ok;
               return run_call(c, dev_, device, stream);
           })

}  // extern "C"
