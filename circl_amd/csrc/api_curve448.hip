// api_curve448.hip -- batch X448 (dh/x448), Ed448 (sign/ed448) and Ed448-Dilithium3 (sign/eddilithium3) behind the C ABI
// (include/circl_hip.h).  No CPU compute path.
#include "ed448_kernels.h"
#include "eddilithium.h"
#include "x448_kernels.h"

using namespace circl::host;

namespace {

// ed448.go ContextMaxSize on the host's offsets: true when some context is longer than 255 bytes
bool context_too_long(const uint8_t *ctx_blob, const uint64_t *ctx_off, size_t n) {
    if (!ctx_blob || !ctx_off) return false;
    for (size_t i = 0; i < n; i++)
        if (ctx_off[i + 1] - ctx_off[i] > 255) return true;
    return false;
}

// X448 KeyGen by the Ed448 comb (x448_dev.h base_mult_comb), the default, or by the ladder from u = 5: CIRCL_HIP_X448_KEYGEN = comb |
// ladder.  The comb is 2.1x the ladder at 2^14 items and 2.2x at 2^18 (profiles/curve448_bench.txt); the ladder stays
// reachable for the comparison.  Like CIRCL_HIP_FRODO_WAVES it is read at every call, so that one process can compare the routes;
// anything but "ladder" is the default.
bool x448_keygen_comb() {
    const char *e = getenv("CIRCL_HIP_X448_KEYGEN");
    return !e || strcmp(e, "ladder") != 0;
}

}  // namespace

namespace circl {
namespace host {
// internal (api_hybrid.hip): out_base[i] = X448(scalar_i, 5) and out_shared[i] = X448(scalar_i, point_i) in one launch
int x448_pair_dev(const uint8_t *d_scalar, const uint8_t *d_point, uint8_t *d_out_base, uint8_t *d_out_shared, uint8_t *d_ok, size_t n,
                  hipStream_t st) {
    if (n == 0) return CIRCL_HIP_OK;
    const unsigned nb = (unsigned)((n + 63) / 64);
    ProfScope ps(CIRCL_HIP_KERNEL_X448, st);
    auto kernel = x448_keygen_comb() ? circl::x448::x448_pair_kernel<true> : circl::x448::x448_pair_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(2 * nb), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar), reinterpret_cast<const uint32_t *>(d_point),
                       reinterpret_cast<uint32_t *>(d_out_base), reinterpret_cast<uint32_t *>(d_out_shared), d_ok, n, nb);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}
}  // namespace host
}  // namespace circl

extern "C" {

// ---- X448 -------------------------------------------------------------------------------------------------------------------
int circl_hip_x448_dev(const uint8_t *d_scalar, const uint8_t *d_point, uint8_t *d_out, uint8_t *d_ok, size_t n, void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (!d_scalar || !d_out) return CIRCL_HIP_EPARAM;
    if (!aligned<4>(d_scalar, d_point, d_out)) return CIRCL_HIP_EWORKSPACE;
    if (n == 0) return CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_X448, st);
    if (d_point)
        hipLaunchKernelGGL((circl::x448::x448_kernel<false, false>), lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar),
                           reinterpret_cast<const uint32_t *>(d_point), reinterpret_cast<uint32_t *>(d_out), d_ok, n);
    else if (x448_keygen_comb())
        hipLaunchKernelGGL((circl::x448::x448_kernel<true, true>), lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar),
                           static_cast<const uint32_t *>(nullptr), reinterpret_cast<uint32_t *>(d_out), d_ok, n);
    else
        hipLaunchKernelGGL((circl::x448::x448_kernel<true, false>), lanes_grid(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar),
                           static_cast<const uint32_t *>(nullptr), reinterpret_cast<uint32_t *>(d_out), d_ok, n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_x448(const uint8_t *scalar, const uint8_t *point, uint8_t *out, uint8_t *ok, size_t n, int device) {
    if (!scalar || !out) return n ? CIRCL_HIP_EPARAM : CIRCL_HIP_OK;
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        std::vector<HIn> ins = {{scalar + lo * 56, 56, true}};
        if (point) ins.push_back({point + lo * 56, 56});
        return run_pipeline(dev, cnt, ins, {}, {{out + lo * 56, 56, true}, {ok ? ok + lo : nullptr, 1}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_x448_dev(c.in[0], point ? c.in[1] : nullptr, c.out[0], c.out[1], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

// ---- Ed448 ------------------------------------------------------------------------------------------------------------------
size_t circl_hip_ed448_workspace_size(size_t n) { return up256(n * circl::ed448::kVerifyWsBytes); }

int circl_hip_ed448_keygen_dev(const uint8_t *d_seed57, uint8_t *d_pk57, uint8_t *d_sk114, size_t n, void *d_workspace, size_t workspace_bytes,
                               void *stream) {
    (void)d_workspace;
    (void)workspace_bytes;  // key generation keeps everything in registers
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_seed57 || (!d_pk57 && !d_sk114)) return CIRCL_HIP_EPARAM;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED448_KEYGEN, st);
    hipLaunchKernelGGL(circl::ed448::ed448_keygen_kernel, lanes_grid(n), dim3(64), 0, st, d_seed57, d_pk57, d_sk114, n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed448_sign_dev(const uint8_t *d_sk114, const uint8_t *d_msg_blob, const uint64_t *d_msg_off, const uint8_t *d_ctx_blob,
                             const uint64_t *d_ctx_off, uint8_t *d_sig114, size_t n, void *d_workspace, size_t workspace_bytes, void *stream) {
    (void)d_workspace;
    (void)workspace_bytes;  // signing keeps every secret in registers: nothing of it reaches the workspace
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_sk114 || !d_msg_off || !d_sig114 || (d_ctx_blob && !d_ctx_off)) return CIRCL_HIP_EPARAM;
    if (!aligned<8>(d_msg_off, d_ctx_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED448_SIGN, st);
    hipLaunchKernelGGL(circl::ed448::ed448_sign_kernel, lanes_grid(n), dim3(64), 0, st, d_sk114, d_msg_blob, d_msg_off, d_ctx_blob, d_ctx_off, d_sig114, n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed448_verify_dev(const uint8_t *d_pk57, const uint8_t *d_sig114, const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                               const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, uint8_t *d_ok, size_t n, void *d_workspace, size_t workspace_bytes,
                               void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_pk57 || !d_sig114 || !d_msg_off || !d_ok || !d_workspace || (d_ctx_blob && !d_ctx_off)) return CIRCL_HIP_EPARAM;
    if (workspace_bytes < circl_hip_ed448_workspace_size(n)) return CIRCL_HIP_EWORKSPACE;
    if (!aligned<4>(d_workspace) || !aligned<8>(d_msg_off, d_ctx_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED448_VERIFY, st);
    hipLaunchKernelGGL(circl::ed448::ed448_verify_prep_kernel, lanes_grid(n), dim3(64), 0, st, d_pk57, d_sig114, d_msg_blob, d_msg_off, d_ctx_blob, d_ctx_off,
                       static_cast<uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(circl::ed448::ed448_verify_kernel, lanes_grid(n), dim3(64), 0, st, d_sig114, d_ok, static_cast<const uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed448_keygen(const uint8_t *seed57, uint8_t *pk57, uint8_t *sk114, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed57 || (!pk57 && !sk114)) return CIRCL_HIP_EPARAM;
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed57 + lo * 57, 57, true}}, {}, {{pk57 ? pk57 + lo * 57 : nullptr, 57}, {sk114 ? sk114 + lo * 114 : nullptr, 114, true}},
                            kNoWs, opts, [&](Chunk &c) { return circl_hip_ed448_keygen_dev(c.in[0], c.out[0], c.out[1], c.cnt, nullptr, 0, c.st); });
    }, kHeavyOneDeviceMax);
}

int circl_hip_ed448_sign(const uint8_t *sk114, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off,
                         uint8_t *sig114, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk114 || !msg_off || !sig114 || (ctx_blob && !ctx_off)) return CIRCL_HIP_EPARAM;
    if (context_too_long(ctx_blob, ctx_off, n)) return CIRCL_HIP_EPARAM;  // the reference panics
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk114 + lo * 114, 114, true}}, {{msg_blob, msg_off + lo}, {ctx_blob, ctx_blob ? ctx_off + lo : nullptr}},
                            {{sig114 + lo * 114, 114}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_ed448_sign_dev(c.in[0], c.blob[0], c.off[0], c.blob[1], c.off[1], c.out[0], c.cnt, nullptr, 0, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_ed448_verify(const uint8_t *pk57, const uint8_t *sig114, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob,
                           const uint64_t *ctx_off, uint8_t *ok, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk57 || !sig114 || !msg_off || !ok || (ctx_blob && !ctx_off)) return CIRCL_HIP_EPARAM;
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 16);  // nothing secret
    const std::function<size_t(size_t)> ws = [](size_t cnt) { return circl_hip_ed448_workspace_size(cnt); };
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk57 + lo * 57, 57}, {sig114 + lo * 114, 114}}, {{msg_blob, msg_off + lo}, {ctx_blob, ctx_blob ? ctx_off + lo : nullptr}},
                            {{ok + lo, 1}}, ws, opts, [&](Chunk &c) {
            return circl_hip_ed448_verify_dev(c.in[0], c.in[1], c.blob[0], c.off[0], c.blob[1], c.off[1], c.out[0], c.cnt, c.ws, c.ws_bytes, c.st);
        });
    }, kHeavyOneDeviceMax);
}

}  // extern "C"

// ---- Ed448-Dilithium3 (sign/eddilithium3): the composition is eddilithium.h's, this is its Ed448 half (with the empty context) ----
static const EdDilithium kEdDilithium3 = {
    3, 1952, 4000, 3293, 57, 57, 114, 114,
    [](const uint8_t *seed, uint8_t *seed_d, uint8_t *seed_e, size_t n, hipStream_t st) -> int {
        hipLaunchKernelGGL(circl::ed448::eddilithium3_seed_kernel, lanes_grid(n), dim3(64), 0, st, seed, reinterpret_cast<uint32_t *>(seed_d), seed_e, n);
        HIP_TRY(hipGetLastError());
        return CIRCL_HIP_OK;
    },
    [](const uint8_t *seed, uint8_t *pk, uint8_t *sk, size_t n, hipStream_t st) { return circl_hip_ed448_keygen_dev(seed, pk, sk, n, nullptr, 0, st); },
    [](const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, hipStream_t st) {
        return circl_hip_ed448_sign_dev(sk, msg_blob, msg_off, nullptr, nullptr, sig, n, nullptr, 0, st);
    },
    [](const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n, void *ws, size_t ws_bytes, hipStream_t st) {
        return circl_hip_ed448_verify_dev(pk, sig, msg_blob, msg_off, nullptr, nullptr, ok, n, ws, ws_bytes, st);
    },
    circl_hip_ed448_workspace_size,
};

extern "C" {

int circl_hip_eddilithium3_keygen(const uint8_t *seed57, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    return eddilithium_keygen(kEdDilithium3, seed57, pk, sk, n, device);
}
int circl_hip_eddilithium3_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device) {
    return eddilithium_sign(kEdDilithium3, sk, msg_blob, msg_off, sig, n, device);
}
int circl_hip_eddilithium3_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n,
                                  int device) {
    return eddilithium_verify(kEdDilithium3, pk, sig, msg_blob, msg_off, ok, n, device);
}

}  // extern "C"
