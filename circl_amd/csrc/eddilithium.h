// eddilithium.h -- the composite signatures of sign/eddilithium2 and sign/eddilithium3: round-3 Dilithium next to an Edwards-curve
// signature, both halves on the device, on the chunk's stream, no host round trip between them.  The composition is written once
// here; api_ed25519.hip and api_curve448.hip each describe their classical half in an EdDilithium next to its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "host_compose.h"

namespace circl {
namespace eddilithium {

// a composite signature is valid when both halves are
static __global__ __launch_bounds__(64) void and_verdicts_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint8_t *__restrict__ ok,
                                                                 size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i < n) ok[i] = (uint8_t)((a[i] != 0) & (b[i] != 0));
}

}  // namespace eddilithium

namespace host {

struct EdDilithium {
    int mode;                        // round-3 Dilithium 2 | 3
    size_t dpk, dsk, dsig;           // its key and signature sizes
    size_t eseed, epk, esk, esig;    // the Edwards half; its packed private key is the seed (eddilithium.go Unpack re-derives the key)
    // the Edwards half on the device, on `st` (every pointer a device pointer)
    int (*split_seed)(const uint8_t *seed, uint8_t *seed_d32, uint8_t *seed_e, size_t n, hipStream_t st);  // the unit's eddilithium*_seed_kernel
    int (*keygen)(const uint8_t *seed, uint8_t *pk, uint8_t *sk, size_t n, hipStream_t st);                // pk or sk may be nullptr
    int (*sign)(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, hipStream_t st);
    int (*verify)(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n, void *ws, size_t ws_bytes,
                  hipStream_t st);
    size_t (*verify_ws)(size_t n);
    size_t pk() const { return dpk + epk; }
    size_t sk() const { return dsk + eseed; }
    size_t sig() const { return dsig + esig; }
};

static inline int eddilithium_keygen(const EdDilithium &d, const uint8_t *seed, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed || !pk || !sk) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [&d](size_t c) {
        return up256(c * 32) + up256(c * d.eseed) + up256(c * d.dpk) + up256(c * d.dsk) + up256(c * d.epk) + circl_hip_mldsa_workspace_size(d.mode, c);
    };
    const PipeOpts opts = secret_opts(size_t(1) << 13);  // the whole workspace is zeroed after every chunk: it holds both seeds
    const size_t PK = d.pk(), SK = d.sk();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed + lo * d.eseed, d.eseed, true}}, {}, {{pk + lo * PK, PK}, {sk + lo * SK, SK, true}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *sd = w.take(c.cnt * 32), *se = w.take(c.cnt * d.eseed), *dpk = w.take(c.cnt * d.dpk), *dsk = w.take(c.cnt * d.dsk),
                    *epk = w.take(c.cnt * d.epk);
            TRY(d.split_seed(c.in[0], sd, se, c.cnt, c.st));
            TRY(circl_hip_mldsa_keygen_dev(d.mode, sd, dpk, dsk, c.cnt, w.rest(), w.left(c.ws_bytes), c.st));
            TRY(d.keygen(se, epk, nullptr, c.cnt, c.st));
            TRY(copy_rows_2d(c.out[0], PK, 0, dpk, d.dpk, 0, d.dpk, c.cnt, c.st));
            TRY(copy_rows_2d(c.out[0], PK, d.dpk, epk, d.epk, 0, d.epk, c.cnt, c.st));
            TRY(copy_rows_2d(c.out[1], SK, 0, dsk, d.dsk, 0, d.dsk, c.cnt, c.st));
            return copy_rows_2d(c.out[1], SK, d.dsk, se, d.eseed, 0, d.eseed, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

static inline int eddilithium_sign(const EdDilithium &d, const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk || !msg_off || !sig) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [&d](size_t c) {
        return up256(c * d.dsk) + up256(c * d.eseed) + up256(c * 32) + up256(c * d.esk) + up256(c * d.esig) + up256(c * d.dsig) +
               circl_hip_mldsa_sign_workspace_size(d.mode, c);
    };
    const PipeOpts opts = secret_opts(size_t(1) << 12);  // the whole workspace is zeroed after every chunk: it holds both private keys
    const size_t SK = d.sk(), SIG = d.sig();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk + lo * SK, SK, true}}, {{msg_blob, msg_off + lo}}, {{sig + lo * SIG, SIG}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dsk = w.take(c.cnt * d.dsk), *se = w.take(c.cnt * d.eseed), *rnd = w.take(c.cnt * 32), *esk = w.take(c.cnt * d.esk),
                    *esig = w.take(c.cnt * d.esig), *dsig = w.take(c.cnt * d.dsig);
            TRY(copy_rows_2d(dsk, d.dsk, 0, c.in[0], SK, 0, d.dsk, c.cnt, c.st));
            TRY(copy_rows_2d(se, d.eseed, 0, c.in[0], SK, d.dsk, d.eseed, c.cnt, c.st));
            HIP_TRY(hipMemsetAsync(rnd, 0, c.cnt * 32, c.st));  // round-3 Dilithium signs deterministically
            TRY(d.keygen(se, nullptr, esk, c.cnt, c.st));       // eddilithium.go Unpack: the Edwards key is re-derived from its seed
            TRY(circl_hip_mldsa_sign_dev(d.mode, dsk, c.blob[0], c.off[0], nullptr, nullptr, rnd, 0, dsig, c.cnt, w.rest(), w.left(c.ws_bytes), c.st));
            TRY(d.sign(esk, c.blob[0], c.off[0], esig, c.cnt, c.st));
            TRY(copy_rows_2d(c.out[0], SIG, 0, dsig, d.dsig, 0, d.dsig, c.cnt, c.st));
            return copy_rows_2d(c.out[0], SIG, d.dsig, esig, d.esig, 0, d.esig, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

static inline int eddilithium_verify(const EdDilithium &d, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok,
                              size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk || !sig || !msg_off || !ok) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [&d](size_t c) {
        return up256(c * d.dpk) + up256(c * d.epk) + up256(c * d.dsig) + up256(c * d.esig) + up256(c) * 2 +
               std::max(circl_hip_mldsa_workspace_size(d.mode, c), d.verify_ws(c));
    };
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 13);  // nothing secret
    const size_t PK = d.pk(), SIG = d.sig();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk + lo * PK, PK}, {sig + lo * SIG, SIG}}, {{msg_blob, msg_off + lo}}, {{ok + lo, 1}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dpk = w.take(c.cnt * d.dpk), *epk = w.take(c.cnt * d.epk), *dsig = w.take(c.cnt * d.dsig), *esig = w.take(c.cnt * d.esig),
                    *ok_d = w.take(c.cnt), *ok_e = w.take(c.cnt);
            TRY(copy_rows_2d(dpk, d.dpk, 0, c.in[0], PK, 0, d.dpk, c.cnt, c.st));
            TRY(copy_rows_2d(epk, d.epk, 0, c.in[0], PK, d.dpk, d.epk, c.cnt, c.st));
            TRY(copy_rows_2d(dsig, d.dsig, 0, c.in[1], SIG, 0, d.dsig, c.cnt, c.st));
            TRY(copy_rows_2d(esig, d.esig, 0, c.in[1], SIG, d.dsig, d.esig, c.cnt, c.st));
            // the two halves run one after the other on the chunk's stream: they share the rest of the workspace
            TRY(circl_hip_mldsa_verify_dev(d.mode, dpk, dsig, c.blob[0], c.off[0], nullptr, nullptr, ok_d, c.cnt, w.rest(), w.left(c.ws_bytes), c.st));
            TRY(d.verify(epk, esig, c.blob[0], c.off[0], ok_e, c.cnt, w.rest(), w.left(c.ws_bytes), c.st));
            hipLaunchKernelGGL(circl::eddilithium::and_verdicts_kernel, lanes_grid(c.cnt), dim3(64), 0, c.st, ok_d, ok_e, c.out[0], c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    }, kHeavyOneDeviceMax);
}

}  // namespace host
}  // namespace circl
