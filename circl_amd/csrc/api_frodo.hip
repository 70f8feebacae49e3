// api_frodo.hip -- batch FrodoKEM-640-SHAKE (kem/frodo/frodo640shake) behind the C ABI (include/circl_hip.h).  No CPU compute path.
#include "frodo_kernels.h"
#include "host_compose.h"

using namespace circl::host;
namespace fr = circl::frodo;

namespace {

// Wavefronts of a matrix workgroup: the 10 row groups of an item are shared by 10, 5 or 2 wavefronts.  10 is the default (DESIGN.md has
// the measurement); CIRCL_HIP_FRODO_WAVES = 5 or 2 selects the others, read at every call so that one process can compare them.
int matrix_waves() {
    const int w = env_int("CIRCL_HIP_FRODO_WAVES", 10, 2, 10);
    return w == 2 || w == 5 ? w : 10;
}
void launch_keygen_matrix(size_t n, hipStream_t st, uint8_t *pk, uint8_t *sk, const uint32_t *noise) {
    switch (matrix_waves()) {
    case 2: hipLaunchKernelGGL(fr::frodo_keygen_matrix_kernel<2>, dim3((unsigned)n), dim3(128), 0, st, pk, sk, noise); break;
    case 5: hipLaunchKernelGGL(fr::frodo_keygen_matrix_kernel<5>, dim3((unsigned)n), dim3(320), 0, st, pk, sk, noise); break;
    default: hipLaunchKernelGGL(fr::frodo_keygen_matrix_kernel<10>, dim3((unsigned)n), dim3(640), 0, st, pk, sk, noise);
    }
}
void launch_encaps_matrix(size_t n, hipStream_t st, const uint8_t *pk, size_t pk_stride, const uint8_t *mu, const uint32_t *noise, uint8_t *out) {
    const size_t mu_stride = fr::kMu, out_stride = fr::kCt;
    switch (matrix_waves()) {
    case 2: hipLaunchKernelGGL(fr::frodo_encaps_matrix_kernel<2>, dim3((unsigned)n), dim3(128), 0, st, pk, pk_stride, mu, mu_stride, noise, out, out_stride); break;
    case 5: hipLaunchKernelGGL(fr::frodo_encaps_matrix_kernel<5>, dim3((unsigned)n), dim3(320), 0, st, pk, pk_stride, mu, mu_stride, noise, out, out_stride); break;
    default: hipLaunchKernelGGL(fr::frodo_encaps_matrix_kernel<10>, dim3((unsigned)n), dim3(640), 0, st, pk, pk_stride, mu, mu_stride, noise, out, out_stride);
    }
}

// a chunk's workspace: the noise rows, k, mu' and the re-encryption, each region 256-byte aligned; all of it is secret
struct Ws {
    uint32_t *noise, *k, *mu, *ct2;
    explicit Ws(void *base, size_t n) {
        uint8_t *p = static_cast<uint8_t *>(base);
        noise = reinterpret_cast<uint32_t *>(p); p += up256(n * fr::kNoiseRow);
        k = reinterpret_cast<uint32_t *>(p);     p += up256(n * 16);
        mu = reinterpret_cast<uint32_t *>(p);    p += up256(n * 16);
        ct2 = reinterpret_cast<uint32_t *>(p);
    }
};
size_t ws_size(size_t n) { return up256(n * fr::kNoiseRow) + 2 * up256(n * 16) + up256(n * fr::kCt); }

int check_ws(const void *ws, size_t bytes, size_t n) {
    if (bytes < ws_size(n) || !aligned<16>(ws)) return CIRCL_HIP_EWORKSPACE;
    return CIRCL_HIP_OK;
}

// rows of 10-20 KB: a chunk of 1024 items is 10240 wavefronts of matrix work (ten per SIMD) and ~60 MB of staging with its workspace
PipeOpts frodo_opts() {
    PipeOpts o;
    o.chunk_items = host_chunk_items(size_t(1) << 10);
    o.depth = 3;
    o.wipe_device = true;
    return o;
}
const std::function<size_t(size_t)> frodo_ws = [](size_t n) { return ws_size(n); };

}  // namespace

extern "C" {

size_t circl_hip_frodo640shake_workspace_size(size_t n) { return ws_size(n); }

int circl_hip_frodo640shake_keygen_dev(const uint8_t *d_seed48, uint8_t *d_pk, uint8_t *d_sk, size_t n, void *d_workspace, size_t workspace_bytes,
                                       void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_seed48 || !d_pk || !d_sk || !d_workspace) return CIRCL_HIP_EPARAM;
    if (int rc = check_ws(d_workspace, workspace_bytes, n)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws w(d_workspace, n);
    {
        ProfScope ps(CIRCL_HIP_KERNEL_FRODO_KEYGEN, st);
        hipLaunchKernelGGL(fr::frodo_keygen_pre_kernel, lanes_grid(n), dim3(64), 0, st, d_seed48, d_pk, d_sk, w.noise, n);
        HIP_TRY(hipGetLastError());
        launch_keygen_matrix(n, st, d_pk, d_sk, w.noise);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(fr::frodo_keygen_post_kernel, lanes_grid(n), dim3(64), 0, st, d_pk, d_sk, n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(d_workspace, 0, ws_size(n), st));  // S, E
    return CIRCL_HIP_OK;
}

int circl_hip_frodo640shake_encaps_dev(const uint8_t *d_pk, const uint8_t *d_seed16, uint8_t *d_ct, uint8_t *d_ss, size_t n, void *d_workspace,
                                       size_t workspace_bytes, void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_pk || !d_seed16 || !d_ct || !d_ss || !d_workspace) return CIRCL_HIP_EPARAM;
    if (int rc = check_ws(d_workspace, workspace_bytes, n)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws w(d_workspace, n);
    {
        ProfScope ps(CIRCL_HIP_KERNEL_FRODO_ENCAPS, st);
        hipLaunchKernelGGL(fr::frodo_encaps_pre_kernel, lanes_grid(n), dim3(64), 0, st, d_pk, d_seed16, w.noise, w.k, n);
        HIP_TRY(hipGetLastError());
        launch_encaps_matrix(n, st, d_pk, fr::kPk, d_seed16, w.noise, d_ct);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(fr::frodo_ss_kernel<false>, lanes_grid(n), dim3(64), 0, st, d_ss, d_ct, w.k, static_cast<const uint32_t *>(nullptr),
                           static_cast<const uint8_t *>(nullptr), n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(d_workspace, 0, ws_size(n), st));  // S', E', E'', k
    return CIRCL_HIP_OK;
}

int circl_hip_frodo640shake_decaps_dev(const uint8_t *d_sk, const uint8_t *d_ct, uint8_t *d_ss, size_t n, void *d_workspace, size_t workspace_bytes,
                                       void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!d_sk || !d_ct || !d_ss || !d_workspace) return CIRCL_HIP_EPARAM;
    if (int rc = check_ws(d_workspace, workspace_bytes, n)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws w(d_workspace, n);
    {
        ProfScope ps(CIRCL_HIP_KERNEL_FRODO_DECAPS, st);
        hipLaunchKernelGGL(fr::frodo_decaps_pre_kernel, lanes_grid(n), dim3(64), 0, st, d_sk, d_ct, w.noise, w.k, w.mu, n);
        HIP_TRY(hipGetLastError());
        // re-encrypt mu' to the pk stored in the key
        launch_encaps_matrix(n, st, d_sk + fr::kSs, fr::kSk, reinterpret_cast<const uint8_t *>(w.mu), w.noise, reinterpret_cast<uint8_t *>(w.ct2));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(fr::frodo_ss_kernel<true>, lanes_grid(n), dim3(64), 0, st, d_ss, d_ct, w.k, w.ct2, d_sk, n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(d_workspace, 0, ws_size(n), st));  // S', E', E'', mu', k', the re-encryption
    return CIRCL_HIP_OK;
}

int circl_hip_frodo640shake_keygen(const uint8_t *seed48, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed48 || !pk || !sk) return CIRCL_HIP_EPARAM;
    const PipeOpts opts = frodo_opts();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed48 + lo * 48, 48, true}}, {}, {{pk + lo * fr::kPk, (size_t)fr::kPk}, {sk + lo * fr::kSk, (size_t)fr::kSk, true}}, frodo_ws,
                            opts, [&](Chunk &c) { return circl_hip_frodo640shake_keygen_dev(c.in[0], c.out[0], c.out[1], c.cnt, c.ws, c.ws_bytes, c.st); });
    }, kHeavyOneDeviceMax);
}

int circl_hip_frodo640shake_encaps(const uint8_t *pk, const uint8_t *seed16, uint8_t *ct, uint8_t *ss, size_t n, int device) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk || !seed16 || !ct || !ss) return CIRCL_HIP_EPARAM;
    const PipeOpts opts = frodo_opts();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk + lo * fr::kPk, (size_t)fr::kPk}, {seed16 + lo * 16, 16, true}}, {},
                            {{ct + lo * fr::kCt, (size_t)fr::kCt}, {ss + lo * 16, 16, true}}, frodo_ws, opts, [&](Chunk &c) {
            return circl_hip_frodo640shake_encaps_dev(c.in[0], c.in[1], c.out[0], c.out[1], c.cnt, c.ws, c.ws_bytes, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_frodo640shake_decaps(const uint8_t *sk, const uint8_t *ct, uint8_t *ss, size_t n, int device) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk || !ct || !ss) return CIRCL_HIP_EPARAM;
    const PipeOpts opts = frodo_opts();
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk + lo * fr::kSk, (size_t)fr::kSk, true}, {ct + lo * fr::kCt, (size_t)fr::kCt}}, {}, {{ss + lo * 16, 16, true}}, frodo_ws, opts,
                            [&](Chunk &c) { return circl_hip_frodo640shake_decaps_dev(c.in[0], c.in[1], c.out[0], c.cnt, c.ws, c.ws_bytes, c.st); });
    }, kHeavyOneDeviceMax);
}

}  // extern "C"
