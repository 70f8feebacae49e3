// api_ed25519.hip -- batch Ed25519 (sign/ed25519) and batch SHA-512 behind the C ABI (include/circl_hip.h).  No CPU compute path.
#include "ed25519_kernels.h"
#include "eddilithium.h"

using namespace circl::host;

extern "C" {

size_t circl_hip_ed25519_workspace_size(size_t n) { return up256(n * circl::ed25519::kVerifyWsBytes); }

int circl_hip_ed25519_keygen_dev(const uint8_t *d_seed32, uint8_t *d_pk32, uint8_t *d_sk64, size_t n, void *d_workspace, size_t workspace_bytes,
                                 void *stream) {
    (void)d_workspace;
    (void)workspace_bytes;  // key generation keeps everything in registers
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_seed32 || (!d_pk32 && !d_sk64)) return CIRCL_HIP_EPARAM;
    if (!aligned<4>(d_seed32, d_pk32, d_sk64)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_KEYGEN, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_keygen_kernel, lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_seed32),
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
    if (!aligned<4>(d_sk64, d_sig64) || !aligned<8>(d_msg_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_SIGN, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_sign_kernel, lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_sk64), d_msg_blob,
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
    if (!aligned<4>(d_pk32, d_sig64, d_workspace) || !aligned<8>(d_msg_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED25519_VERIFY, st);
    hipLaunchKernelGGL(circl::ed25519::ed25519_verify_prep_kernel, lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_pk32),
                       reinterpret_cast<const uint32_t *>(d_sig64), d_msg_blob, d_msg_off, static_cast<uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(circl::ed25519::ed25519_verify_kernel, lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_sig64), d_ok,
                       static_cast<const uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed25519_keygen(const uint8_t *seed32, uint8_t *pk32, uint8_t *sk64, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed32 || (!pk32 && !sk64)) return CIRCL_HIP_EPARAM;
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed32 + lo * 32, 32, true}}, {}, {{pk32 ? pk32 + lo * 32 : nullptr, 32}, {sk64 ? sk64 + lo * 64 : nullptr, 64, true}},
                            kNoWs, secret_opts(size_t(1) << 16), [&](Chunk &c) { return circl_hip_ed25519_keygen_dev(c.in[0], c.out[0], c.out[1], c.cnt, nullptr, 0, c.st); });
    }, kHeavyOneDeviceMax);
}

int circl_hip_ed25519_sign(const uint8_t *sk64, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig64, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk64 || !msg_off || !sig64) return CIRCL_HIP_EPARAM;
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk64 + lo * 64, 64, true}}, {{msg_blob, msg_off + lo}}, {{sig64 + lo * 64, 64}}, kNoWs, secret_opts(size_t(1) << 16), [&](Chunk &c) {
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
        return run_pipeline(dev, cnt, {}, {{msg_blob, msg_off + lo}}, {{out64 + lo * 64, 64}}, kNoWs, opts, [&](Chunk &c) {
            ProfScope ps(CIRCL_HIP_KERNEL_SHA512, c.st);
            hipLaunchKernelGGL(circl::ed25519::sha512_kernel, lanes_grid(c.cnt), dim3(64), 0, c.st, c.blob[0], c.off[0], reinterpret_cast<uint32_t *>(c.out[0]),
                               c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    });
}

}  // extern "C"

// ---- Ed25519-Dilithium2 (sign/eddilithium2): the composition is eddilithium.h's, this is its Ed25519 half ----
static const EdDilithium kEdDilithium2 = {
    2, 1312, 2528, 2420, 32, 32, 64, 64,
    [](const uint8_t *seed, uint8_t *seed_d, uint8_t *seed_e, size_t n, hipStream_t st) -> int {
        hipLaunchKernelGGL(circl::ed25519::eddilithium2_seed_kernel, lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(seed),
                           reinterpret_cast<uint32_t *>(seed_d), reinterpret_cast<uint32_t *>(seed_e), n);
        HIP_TRY(hipGetLastError());
        return CIRCL_HIP_OK;
    },
    [](const uint8_t *seed, uint8_t *pk, uint8_t *sk, size_t n, hipStream_t st) { return circl_hip_ed25519_keygen_dev(seed, pk, sk, n, nullptr, 0, st); },
    [](const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, hipStream_t st) {
        return circl_hip_ed25519_sign_dev(sk, msg_blob, msg_off, sig, n, nullptr, 0, st);
    },
    [](const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n, void *ws, size_t ws_bytes, hipStream_t st) {
        return circl_hip_ed25519_verify_dev(pk, sig, msg_blob, msg_off, ok, n, ws, ws_bytes, st);
    },
    circl_hip_ed25519_workspace_size,
};

extern "C" {

int circl_hip_eddilithium2_keygen(const uint8_t *seed32, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    return eddilithium_keygen(kEdDilithium2, seed32, pk, sk, n, device);
}
int circl_hip_eddilithium2_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device) {
    return eddilithium_sign(kEdDilithium2, sk, msg_blob, msg_off, sig, n, device);
}
int circl_hip_eddilithium2_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n,
                                  int device) {
    return eddilithium_verify(kEdDilithium2, pk, sig, msg_blob, msg_off, ok, n, device);
}

}  // extern "C"
