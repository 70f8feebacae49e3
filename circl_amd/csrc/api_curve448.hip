// api_curve448.hip -- batch X448 (dh/x448), Ed448 (sign/ed448) and Ed448-Dilithium3 (sign/eddilithium3) behind the C ABI
// (include/circl_hip.h).  No CPU compute path.
#include "ed448_kernels.h"
#include "host_common.h"
#include "x448_kernels.h"

using namespace circl::host;

namespace {

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
dim3 grid_of(size_t n) { return dim3((unsigned)((n + 63) / 64)); }
const std::function<size_t(size_t)> no_ws = [](size_t) { return size_t(0); };

PipeOpts secret_opts(size_t chunk) {
    PipeOpts o;
    o.chunk_items = host_chunk_items(chunk);
    o.wipe_device = true;  // seeds, private keys, shared secrets
    return o;
}

// ed448.go ContextMaxSize on the host's offsets: true when some context is longer than 255 bytes
bool context_too_long(const uint8_t *ctx_blob, const uint64_t *ctx_off, size_t n) {
    if (!ctx_blob || !ctx_off) return false;
    for (size_t i = 0; i < n; i++)
        if (ctx_off[i + 1] - ctx_off[i] > 255) return true;
    return false;
}

}  // namespace

extern "C" {

// ---- X448 -------------------------------------------------------------------------------------------------------------------
int circl_hip_x448_dev(const uint8_t *d_scalar, const uint8_t *d_point, uint8_t *d_out, uint8_t *d_ok, size_t n, void *stream) {
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    if (!d_scalar || !d_out) return CIRCL_HIP_EPARAM;
    if (!aligned4(d_scalar) || !aligned4(d_point) || !aligned4(d_out)) return CIRCL_HIP_EWORKSPACE;
    if (n == 0) return CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_X448, st);
    if (d_point)
        hipLaunchKernelGGL(circl::x448::x448_kernel<false>, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar),
                           reinterpret_cast<const uint32_t *>(d_point), reinterpret_cast<uint32_t *>(d_out), d_ok, n);
    else
        hipLaunchKernelGGL(circl::x448::x448_kernel<true>, grid_of(n), dim3(64), 0, st, reinterpret_cast<const uint32_t *>(d_scalar),
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
        return run_pipeline(dev, cnt, ins, {}, {{out + lo * 56, 56, true}, {ok ? ok + lo : nullptr, 1}}, no_ws, opts, [&](Chunk &c) {
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
    hipLaunchKernelGGL(circl::ed448::ed448_keygen_kernel, grid_of(n), dim3(64), 0, st, d_seed57, d_pk57, d_sk114, n);
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
    if (!aligned8(d_msg_off) || !aligned8(d_ctx_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED448_SIGN, st);
    hipLaunchKernelGGL(circl::ed448::ed448_sign_kernel, grid_of(n), dim3(64), 0, st, d_sk114, d_msg_blob, d_msg_off, d_ctx_blob, d_ctx_off, d_sig114, n);
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
    if (!aligned4(d_workspace) || !aligned8(d_msg_off) || !aligned8(d_ctx_off)) return CIRCL_HIP_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps(CIRCL_HIP_KERNEL_ED448_VERIFY, st);
    hipLaunchKernelGGL(circl::ed448::ed448_verify_prep_kernel, grid_of(n), dim3(64), 0, st, d_pk57, d_sig114, d_msg_blob, d_msg_off, d_ctx_blob, d_ctx_off,
                       static_cast<uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(circl::ed448::ed448_verify_kernel, grid_of(n), dim3(64), 0, st, d_sig114, d_ok, static_cast<const uint32_t *>(d_workspace), n);
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

int circl_hip_ed448_keygen(const uint8_t *seed57, uint8_t *pk57, uint8_t *sk114, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed57 || (!pk57 && !sk114)) return CIRCL_HIP_EPARAM;
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed57 + lo * 57, 57, true}}, {}, {{pk57 ? pk57 + lo * 57 : nullptr, 57}, {sk114 ? sk114 + lo * 114 : nullptr, 114, true}},
                            no_ws, opts, [&](Chunk &c) { return circl_hip_ed448_keygen_dev(c.in[0], c.out[0], c.out[1], c.cnt, nullptr, 0, c.st); });
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
                            {{sig114 + lo * 114, 114}}, no_ws, opts, [&](Chunk &c) {
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

// ---- Ed448-Dilithium3 (sign/eddilithium3): both halves on the device, on the chunk's stream, no host round trip between them ----
namespace {
constexpr size_t kDPk = 1952, kDSk = 4000, kDSig = 3293, kEdPk = kDPk + 57, kEdSk = kDSk + 57, kEdSig = kDSig + 114;

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

int circl_hip_eddilithium3_keygen(const uint8_t *seed57, uint8_t *pk, uint8_t *sk, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!seed57 || !pk || !sk) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * 32) + up256(c * 57) + up256(c * kDPk) + up256(c * kDSk) + up256(c * 57) + circl_hip_mldsa_workspace_size(3, c);
    };
    const PipeOpts opts = secret_opts(size_t(1) << 13);  // the whole workspace is zeroed after every chunk: it holds both seeds
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{seed57 + lo * 57, 57, true}}, {}, {{pk + lo * kEdPk, kEdPk}, {sk + lo * kEdSk, kEdSk, true}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *sd = w.take(c.cnt * 32), *se = w.take(c.cnt * 57), *dpk = w.take(c.cnt * kDPk), *dsk = w.take(c.cnt * kDSk),
                    *epk = w.take(c.cnt * 57);
            const size_t rest = c.ws_bytes - w.at;
            hipLaunchKernelGGL(circl::ed448::eddilithium3_seed_kernel, grid_of(c.cnt), dim3(64), 0, c.st, c.in[0], reinterpret_cast<uint32_t *>(sd), se, c.cnt);
            HIP_TRY(hipGetLastError());
            int rc = circl_hip_mldsa_keygen_dev(3, sd, dpk, dsk, c.cnt, w.base + w.at, rest, c.st);
            if (rc) return rc;
            if ((rc = circl_hip_ed448_keygen_dev(se, epk, nullptr, c.cnt, nullptr, 0, c.st))) return rc;
            if ((rc = copy_rows(c.out[0], kEdPk, 0, dpk, kDPk, 0, kDPk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(c.out[0], kEdPk, kDPk, epk, 57, 0, 57, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(c.out[1], kEdSk, 0, dsk, kDSk, 0, kDSk, c.cnt, c.st))) return rc;
            return copy_rows(c.out[1], kEdSk, kDSk, se, 57, 0, 57, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_eddilithium3_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!sk || !msg_off || !sig) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * kDSk) + up256(c * 57) + up256(c * 32) + up256(c * 114) * 2 + up256(c * kDSig) + circl_hip_mldsa_sign_workspace_size(3, c);
    };
    const PipeOpts opts = secret_opts(size_t(1) << 12);  // the whole workspace is zeroed after every chunk: it holds both private keys
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{sk + lo * kEdSk, kEdSk, true}}, {{msg_blob, msg_off + lo}}, {{sig + lo * kEdSig, kEdSig}}, ws, opts, [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dsk = w.take(c.cnt * kDSk), *se = w.take(c.cnt * 57), *rnd = w.take(c.cnt * 32), *esk = w.take(c.cnt * 114),
                    *esig = w.take(c.cnt * 114), *dsig = w.take(c.cnt * kDSig);
            const size_t rest = c.ws_bytes - w.at;
            int rc;
            if ((rc = copy_rows(dsk, kDSk, 0, c.in[0], kEdSk, 0, kDSk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(se, 57, 0, c.in[0], kEdSk, kDSk, 57, c.cnt, c.st))) return rc;
            HIP_TRY(hipMemsetAsync(rnd, 0, c.cnt * 32, c.st));  // round-3 Dilithium3 signs deterministically
            // eddilithium.go Unpack: the Ed448 key is re-derived from its seed
            if ((rc = circl_hip_ed448_keygen_dev(se, nullptr, esk, c.cnt, nullptr, 0, c.st))) return rc;
            if ((rc = circl_hip_mldsa_sign_dev(3, dsk, c.blob[0], c.off[0], nullptr, nullptr, rnd, 0, dsig, c.cnt, w.base + w.at, rest, c.st))) return rc;
            if ((rc = circl_hip_ed448_sign_dev(esk, c.blob[0], c.off[0], nullptr, nullptr, esig, c.cnt, nullptr, 0, c.st))) return rc;  // empty context
            if ((rc = copy_rows(c.out[0], kEdSig, 0, dsig, kDSig, 0, kDSig, c.cnt, c.st))) return rc;
            return copy_rows(c.out[0], kEdSig, kDSig, esig, 114, 0, 114, c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_eddilithium3_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok, size_t n,
                                  int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!pk || !sig || !msg_off || !ok) return CIRCL_HIP_EPARAM;
    const std::function<size_t(size_t)> ws = [](size_t c) {
        return up256(c * kDPk) + up256(c * 57) + up256(c * kDSig) + up256(c * 114) + up256(c) * 2 +
               std::max(circl_hip_mldsa_workspace_size(3, c), circl_hip_ed448_workspace_size(c));
    };
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 13);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pk + lo * kEdPk, kEdPk}, {sig + lo * kEdSig, kEdSig}}, {{msg_blob, msg_off + lo}}, {{ok + lo, 1}}, ws, opts,
                            [&](Chunk &c) {
            Carve w{c.ws};
            uint8_t *dpk = w.take(c.cnt * kDPk), *epk = w.take(c.cnt * 57), *dsig = w.take(c.cnt * kDSig), *esig = w.take(c.cnt * 114),
                    *ok_d = w.take(c.cnt), *ok_e = w.take(c.cnt);
            const size_t rest = c.ws_bytes - w.at;
            int rc;
            if ((rc = copy_rows(dpk, kDPk, 0, c.in[0], kEdPk, 0, kDPk, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(epk, 57, 0, c.in[0], kEdPk, kDPk, 57, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(dsig, kDSig, 0, c.in[1], kEdSig, 0, kDSig, c.cnt, c.st))) return rc;
            if ((rc = copy_rows(esig, 114, 0, c.in[1], kEdSig, kDSig, 114, c.cnt, c.st))) return rc;
            if ((rc = circl_hip_mldsa_verify_dev(3, dpk, dsig, c.blob[0], c.off[0], nullptr, nullptr, ok_d, c.cnt, w.base + w.at, rest, c.st))) return rc;
            if ((rc = circl_hip_ed448_verify_dev(epk, esig, c.blob[0], c.off[0], nullptr, nullptr, ok_e, c.cnt, w.base + w.at, rest, c.st))) return rc;
            hipLaunchKernelGGL(circl::ed448::and_verdicts448_kernel, grid_of(c.cnt), dim3(64), 0, c.st, ok_d, ok_e, c.out[0], c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    }, kHeavyOneDeviceMax);
}

}  // extern "C"
