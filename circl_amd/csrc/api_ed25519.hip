// api_ed25519.hip -- batch Ed25519 (sign/ed25519) and batch SHA-512 behind the C ABI (include/circl_hip.h).  No CPU compute path.
#include "ed25519_kernels.h"
#include "host_common.h"

using namespace circl::host;

namespace {

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
dim3 grid_of(size_t n) { return dim3((unsigned)((n + 63) / 64)); }
const std::function<size_t(size_t)> no_ws = [](size_t) { return size_t(0); };

PipeOpts ed_opts() {
    PipeOpts o;
    o.chunk_items = host_chunk_items(size_t(1) << 16);
    o.wipe_device = true;  // seeds, private keys
    return o;
}

}  // namespace

extern "C" {

size_t circl_hip_ed25519_workspace_size(size_t n) { return up256(n * circl::ed25519::kVerifyWsBytes); }

int circl_hip_ed25519_keygen_dev(const uint8_t *d_seed32, uint8_t *d_pk32, uint8_t *d_sk64, size_t n, void *d_workspace, size_t workspace_bytes,
                                 void *stream) {
    (void)d_workspace;
    (void)workspace_bytes;  // key generation keeps everything in registers
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_seed32 || (!d_pk32 && !d_sk64)) return CIRCL_HIP_EPARAM;
    if (!aligned4(d_seed32) || !aligned4(d_pk32) || !aligned4(d_sk64)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_KEYGEN, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_keygen_kernel, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_seed32),
                       reinterpret_cast<uint32_t *>(d_pk32), reinterpret_cast<uint32_t *>(d_sk64), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed25519_sign_dev(const uint8_t *d_sk64, const uint8_t *d_msg_blob, const uint64_t *d_msg_off, uint8_t *d_sig64, size_t n,
                               void *d_workspace, size_t workspace_bytes, void *stream) {
    (void)d_workspace;
    (void)workspace_bytes;  // signing keeps every secret in registers: nothing of it reaches the workspace
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_sk64 || !d_msg_off || !d_sig64) return CIRCL_HIP_EPARAM;
    if (!aligned4(d_sk64) || !aligned4(d_sig64) || (reinterpret_cast<uintptr_t>(d_msg_off) & 7)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_SIGN, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_sign_kernel, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_sk64), d_msg_blob,
                       d_msg_off, reinterpret_cast<uint32_t *>(d_sig64), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed25519_verify_dev(const uint8_t *d_pk32, const uint8_t *d_sig64, const uint8_t *d_msg_blob, const uint64_t *d_msg_off, uint8_t *d_ok,
                                 size_t n, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_pk32 || !d_sig64 || !d_msg_off || !d_ok || !d_workspace) return CIRCL_HIP_EPARAM;
    if (workspace_bytes < circl_hip_ed25519_workspace_size(n)) return CIRCL_HIP_EWORKSPACE;
    if (!aligned4(d_pk32) || !aligned4(d_sig64) || !aligned4(d_workspace) || (reinterpret_cast<uintptr_t>(d_msg_off) & 7)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_VERIFY, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_verify_prep_kernel, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_pk32),
                       reinterpret_cast<const uint32_t *>(d_sig64), d_msg_blob, d_msg_off, static_cast<uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(circl::ed25519::ed25519_verify_kernel, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_sig64), d_ok,
                       static_cast<const uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed25519_keygen(const uint8_t *seed32, uint8_t *pk32, uint8_t *sk64, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed32 || (!pk32 && !sk64)) return CIRCL_HIP_EPARAM;
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed32 + lo * 32, 32, true}}, {}, {{pk32 ? pk32 + lo * 32 : nullptr, 32}, {sk64 ? sk64 + lo * 64 : nullptr, 64, true}},
                            no_ws, ed_opts(), [&](Chunk &c) { return circl_hip_ed25519_keygen_dev(c.in[0], c.out[0], c.out[1], c.cnt, nullptr, 0, c.st); });
    }, kHeavyOneDeviceMax);
}

int circl_hip_ed25519_sign(const uint8_t *sk64, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig64, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk64 || !msg_off || !sig64) return CIRCL_HIP_EPARAM;
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk64 + lo * 64, 64, true}}, {{msg_blob, msg_off + lo}}, {{sig64 + lo * 64, 64}}, no_ws, ed_opts(), [&](Chunk &c) {
            return circl_hip_ed25519_sign_dev(c.in[0], c.blob[0], c.off[0], c.out[0], c.cnt, nullptr, 0, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_ed25519_verify(const uint8_t *pk32, const uint8_t *sig64, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n,
                             int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk32 || !sig64 || !msg_off || !ok) return CIRCL_HIP_EPARAM;
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 16);  // nothing secret
    const std::function<size_t(size_t)> ws = [](size_t cnt) { return circl_hip_ed25519_workspace_size(cnt); };
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk32 + lo * 32, 32}, {sig64 + lo * 64, 64}}, {{msg_blob, msg_off + lo}}, {{ok + lo, 1}}, ws, opts, [&](Chunk &c) {
            return circl_hip_ed25519_verify_dev(c.in[0], c.in[1], c.blob[0], c.off[0], c.out[0], c.cnt, c.ws, c.ws_bytes, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_sha512(const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *out64, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!msg_off || !out64) return CIRCL_HIP_EPARAM;
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {}, {{msg_blob, msg_off + lo}}, {{out64 + lo * 64, 64}}, no_ws, opts, [&](Chunk &c) {
            ProfScope ps(CIRCL_HIP_KERNEL_SHA512, c.st);
            hipLaunchKernelGGL(circl::ed25519::sha512_kernel, grid_of(c.cnt), dim3(64), 0, c.st, c.blob[0], c.off[0], reinterpret_cast<uint32_t *>(c.out[0]),
                               c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    });
}

}  // extern "C"

// ---- Ed25519-Dilithium2 (sign/eddilithium2): both halves on the device, on the chunk's stream, no host round trip between them ----
namespace {
constexpr size_t kDPk = 1312, kDSk = 2528, kDSig = 2420, kEdPk = kDPk + 32, kEdSk = kDSk + 32, kEdSig = kDSig + 64;

// strided device-to-device row copies: columns [src_col, src_col + w) of rows of src_pitch -> columns [dst_col, ..) of rows of dst_pitch
int copy_rows(uint8_t *dst, size_t dst_pitch, size_t dst_col, const uint8_t *src, size_t src_pitch, size_t src_col, size_t w, size_t rows,
              hipStream_t st) {
    HIP_TRY(hipMemcpy2DAsync(dst + dst_col, dst_pitch, src + src_col, src_pitch, w, rows, hipMemcpyDeviceToDevice, st));
    return CIRCL_HIP_OK;
}

struct Carve {  // consecutive 256-byte-aligned regions of a chunk's workspace
    uint8_t *base;
    size_t at = 0;
    uint8_t *take(size_t bytes) {
        uint8_t *p = base + at;
        at += up256(bytes);
        return p;
    }
};
}  // namespace

extern "C" {

int circl_hip_eddilithium2_keygen(const uint8_t *seed32, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed32 || !pk || !sk) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * 32) * 2 + up256(c * kDPk) + up256(c * kDSk) + up256(c * 32) + circl_hip_mldsa_workspace_size(2, c);
    };
    PipeOpts opts = ed_opts();
    opts.chunk_items = host_chunk_items(size_t(1) << 13);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed32 + lo * 32, 32, true}}, {}, {{pk + lo * kEdPk, kEdPk}, {sk + lo * kEdSk, kEdSk, true}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *sd = w.take(c.cnt * 32), *se = w.take(c.cnt * 32), *dpk = w.take(c.cnt * kDPk), *dsk = w.take(c.cnt * kDSk),
                    *epk = w.take(c.cnt * 32);
            const size_t rest = c.ws_bytes - w.at;
            hipLaunchKernelGGL(circl::ed25519::eddilithium2_seed_kernel, grid_of(c.cnt), dim3(64), 0, c.st, reinterpret_cast<const uint32_t *>(c.in[0]),
                               reinterpret_cast<uint32_t *>(sd), reinterpret_cast<uint32_t *>(se), c.cnt);
            HIP_TRY(hipGetLastError());
            int rc = circl_hip_mldsa_keygen_dev(2, sd, dpk, dsk, c.cnt, w.base + w.at, rest, c.st);
            if (rc) return rc;
            if ((rc = circl_hip_ed25519_keygen_dev(se, epk, nullptr, c.cnt, nullptr, 0, c.st))) return rc;
            if ((rc = copy_rows(c.out[0], kEdPk, 0, dpk, kDPk, 0, kDPk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(c.out[0], kEdPk, kDPk, epk, 32, 0, 32, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(c.out[1], kEdSk, 0, dsk, kDSk, 0, kDSk, c.cnt, c.st))) return rc;
            return copy_rows(c.out[1], kEdSk, kDSk, se, 32, 0, 32, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_eddilithium2_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk || !msg_off || !sig) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * kDSk) + up256(c * 32) * 2 + up256(c * 64) * 2 + up256(c * kDSig) + circl_hip_mldsa_sign_workspace_size(2, c);
    };
    PipeOpts opts = ed_opts();  // the whole workspace is zeroed after every chunk: it holds both private keys
    opts.chunk_items = host_chunk_items(size_t(1) << 12);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk + lo * kEdSk, kEdSk, true}}, {{msg_blob, msg_off + lo}}, {{sig + lo * kEdSig, kEdSig}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dsk = w.take(c.cnt * kDSk), *se = w.take(c.cnt * 32), *rnd = w.take(c.cnt * 32), *esk = w.take(c.cnt * 64),
                    *esig = w.take(c.cnt * 64), *dsig = w.take(c.cnt * kDSig);
            const size_t rest = c.ws_bytes - w.at;
            int rc;
            if ((rc = copy_rows(dsk, kDSk, 0, c.in[0], kEdSk, 0, kDSk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(se, 32, 0, c.in[0], kEdSk, kDSk, 32, c.cnt, c.st))) return rc;
            HIP_TRY(hipMemsetAsync(rnd, 0, c.cnt * 32, c.st));  // round-3 Dilithium2 signs deterministically
            // eddilithium.go Unpack (:127-132): the Ed25519 key is re-derived from its seed
            if ((rc = circl_hip_ed25519_keygen_dev(se, nullptr, esk, c.cnt, nullptr, 0, c.st))) return rc;
            if ((rc = circl_hip_mldsa_sign_dev(2, dsk, c.blob[0], c.off[0], nullptr, nullptr, rnd, 0, dsig, c.cnt, w.base + w.at, rest, c.st))) return rc;
            if ((rc = circl_hip_ed25519_sign_dev(esk, c.blob[0], c.off[0], esig, c.cnt, nullptr, 0, c.st))) return rc;
            if ((rc = copy_rows(c.out[0], kEdSig, 0, dsig, kDSig, 0, kDSig, c.cnt, c.st))) return rc;
            return copy_rows(c.out[0], kEdSig, kDSig, esig, 64, 0, 64, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_eddilithium2_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n,
                                  int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk || !sig || !msg_off || !ok) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * kDPk) + up256(c * 32) + up256(c * kDSig) + up256(c * 64) + up256(c) * 2 +
               std::max(circl_hip_mldsa_workspace_size(2, c), circl_hip_ed25519_workspace_size(c));
    };
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 13);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk + lo * kEdPk, kEdPk}, {sig + lo * kEdSig, kEdSig}}, {{msg_blob, msg_off + lo}}, {{ok + lo, 1}}, ws, opts,
                            [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dpk = w.take(c.cnt * kDPk), *epk = w.take(c.cnt * 32), *dsig = w.take(c.cnt * kDSig), *esig = w.take(c.cnt * 64),
                    *ok_d = w.take(c.cnt), *ok_e = w.take(c.cnt);
            const size_t rest = c.ws_bytes - w.at;
            int rc;
            if ((rc = copy_rows(dpk, kDPk, 0, c.in[0], kEdPk, 0, kDPk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(epk, 32, 0, c.in[0], kEdPk, kDPk, 32, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(dsig, kDSig, 0, c.in[1], kEdSig, 0, kDSig, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(esig, 64, 0, c.in[1], kEdSig, kDSig, 64, c.cnt, c.st))) return rc;
            if ((rc = circl_hip_mldsa_verify_dev(2, dpk, dsig, c.blob[0], c.off[0], nullptr, nullptr, ok_d, c.cnt, w.base + w.at, rest, c.st))) return rc;
            if ((rc = circl_hip_ed25519_verify_dev(epk, esig, c.blob[0], c.off[0], ok_e, c.cnt, w.base + w.at, rest, c.st))) return rc;
            hipLaunchKernelGGL(circl::ed25519::and_verdicts_kernel, grid_of(c.cnt), dim3(64), 0, c.st, ok_d, ok_e, c.out[0], c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    }, kHeavyOneDeviceMax);
}

}  // extern "C"
