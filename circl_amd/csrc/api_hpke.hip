// api_hpke.hip -- batch HPKE DHKEM over X25519 / HKDF-SHA256 (KEM id 0x20) and X448 / HKDF-SHA512 (0x21) (hpke/kembase.go,
// hpke/xkem.go) and the batch SHA-256 primitive behind the C ABI (include/circl_hip.h).  No CPU compute path.
#include "dhkem_kernels.h"
#include "host_compose.h"

using namespace circl::host;
using circl::dhkem::X25519;
using circl::dhkem::X448;

namespace {

bool kem_known(int kem) { return kem == 0x20 || kem == 0x21; }
size_t key_bytes(int kem) { return kem == 0x20 ? 32 : kem == 0x21 ? 56 : 0; }
size_t ss_bytes(int kem) { return kem == 0x20 ? 32 : kem == 0x21 ? 64 : 0; }

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *w(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

// the argument contract of a _dev form, checked before any device is looked for; 1 = nothing to do (n == 0)
template <class... P>
int dev_args(int kem, bool have_all, size_t n, P... p) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return 1;
    if (!have_all) return CIRCL_HIP_EPARAM;
    if (!aligned<4>(p...)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    return CIRCL_HIP_OK;
}

}  // namespace

#define DHKEM_LAUNCH(kernel, ...)                                                                                                       \
    do {                                                                                                                                \
        ProfScope ps(kem == 0x20 ? CIRCL_HIP_KERNEL_HPKE_X25519 : CIRCL_HIP_KERNEL_HPKE_X448, st);                                      \
        if (kem == 0x20) hipLaunchKernelGGL(circl::dhkem::kernel<X25519>, lanes_grid(n), dim3(64), 0, st, __VA_ARGS__);                 \
        else hipLaunchKernelGGL(circl::dhkem::kernel<X448>, lanes_grid(n), dim3(64), 0, st, __VA_ARGS__);                               \
        HIP_TRY(hipGetLastError());                                                                                                     \
        return CIRCL_HIP_OK;                                                                                                            \
    } while (0)

extern "C" {

size_t circl_hip_hpke_dhkem_key_size(int kem) { return key_bytes(kem); }
size_t circl_hip_hpke_dhkem_ss_size(int kem) { return ss_bytes(kem); }

// ---- device-resident forms ---------------------------------------------------------------------------------------------------
int circl_hip_hpke_dhkem_derive_keypair_dev(int kem, const uint8_t *d_ikm, uint8_t *d_sk, uint8_t *d_pk, size_t n, void *stream) {
    if (int rc = dev_args(kem, d_ikm && d_sk && d_pk, n, d_ikm, d_sk, d_pk)) return rc < 0 ? rc : CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DHKEM_LAUNCH(derive_keypair_kernel, w(d_ikm), w(d_sk), w(d_pk), n);
}

int circl_hip_hpke_dhkem_encap_dev(int kem, const uint8_t *d_pkR, const uint8_t *d_ikmE, uint8_t *d_enc, uint8_t *d_ss, uint8_t *d_ok, size_t n,
                                   void *stream) {
    if (int rc = dev_args(kem, d_pkR && d_ikmE && d_enc && d_ss, n, d_pkR, d_ikmE, d_enc, d_ss)) return rc < 0 ? rc : CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DHKEM_LAUNCH(encap_kernel, w(d_pkR), w(d_ikmE), w(d_enc), w(d_ss), d_ok, n);
}

int circl_hip_hpke_dhkem_decap_dev(int kem, const uint8_t *d_skR, const uint8_t *d_pkR, const uint8_t *d_enc, uint8_t *d_ss, uint8_t *d_ok, size_t n,
                                   void *stream) {
    if (int rc = dev_args(kem, d_skR && d_enc && d_ss, n, d_skR, d_pkR, d_enc, d_ss)) return rc < 0 ? rc : CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DHKEM_LAUNCH(decap_kernel, w(d_skR), w(d_pkR), w(d_enc), w(d_ss), d_ok, n);
}

int circl_hip_hpke_dhkem_auth_encap_dev(int kem, const uint8_t *d_pkR, const uint8_t *d_skS, const uint8_t *d_pkS, const uint8_t *d_ikmE, uint8_t *d_enc,
                                        uint8_t *d_ss, uint8_t *d_ok, size_t n, void *stream) {
    if (int rc = dev_args(kem, d_pkR && d_skS && d_ikmE && d_enc && d_ss, n, d_pkR, d_skS, d_pkS, d_ikmE, d_enc, d_ss)) return rc < 0 ? rc : CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DHKEM_LAUNCH(auth_encap_kernel, w(d_pkR), w(d_skS), w(d_pkS), w(d_ikmE), w(d_enc), w(d_ss), d_ok, n);
}

int circl_hip_hpke_dhkem_auth_decap_dev(int kem, const uint8_t *d_skR, const uint8_t *d_pkR, const uint8_t *d_enc, const uint8_t *d_pkS, uint8_t *d_ss,
                                        uint8_t *d_ok, size_t n, void *stream) {
    if (int rc = dev_args(kem, d_skR && d_enc && d_pkS && d_ss, n, d_skR, d_pkR, d_enc, d_pkS, d_ss)) return rc < 0 ? rc : CIRCL_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DHKEM_LAUNCH(auth_decap_kernel, w(d_skR), w(d_pkR), w(d_enc), w(d_pkS), w(d_ss), d_ok, n);
}

// ---- host-buffer forms: sharded over the devices, staged through the pipeline, the staging of every secret row wiped ---------
int circl_hip_hpke_dhkem_derive_keypair(int kem, const uint8_t *ikm, uint8_t *sk, uint8_t *pk, size_t n, int device) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return CIRCL_HIP_OK;
    if (!ikm || !sk || !pk) return CIRCL_HIP_EPARAM;
    const size_t N = key_bytes(kem);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{ikm + lo * N, N, true}}, {}, {{sk + lo * N, N, true}, {pk + lo * N, N}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_hpke_dhkem_derive_keypair_dev(kem, c.in[0], c.out[0], c.out[1], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_hpke_dhkem_encap(int kem, const uint8_t *pkR, const uint8_t *ikmE, uint8_t *enc, uint8_t *ss, uint8_t *ok, size_t n, int device) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return CIRCL_HIP_OK;
    if (!pkR || !ikmE || !enc || !ss) return CIRCL_HIP_EPARAM;
    const size_t N = key_bytes(kem), S = ss_bytes(kem);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {{pkR + lo * N, N}, {ikmE + lo * N, N, true}}, {}, {{enc + lo * N, N}, {ss + lo * S, S, true}, {ok ? ok + lo : nullptr, 1}},
                            kNoWs, opts, [&](Chunk &c) {
            return circl_hip_hpke_dhkem_encap_dev(kem, c.in[0], c.in[1], c.out[0], c.out[1], c.out[2], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_hpke_dhkem_decap(int kem, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, uint8_t *ss, uint8_t *ok, size_t n, int device) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return CIRCL_HIP_OK;
    if (!skR || !enc || !ss) return CIRCL_HIP_EPARAM;
    const size_t N = key_bytes(kem), S = ss_bytes(kem);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        std::vector<HIn> ins = {{skR + lo * N, N, true}, {enc + lo * N, N}};
        if (pkR) ins.push_back({pkR + lo * N, N});
        return run_pipeline(dev, cnt, ins, {}, {{ss + lo * S, S, true}, {ok ? ok + lo : nullptr, 1}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_hpke_dhkem_decap_dev(kem, c.in[0], pkR ? c.in[2] : nullptr, c.in[1], c.out[0], c.out[1], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_hpke_dhkem_auth_encap(int kem, const uint8_t *pkR, const uint8_t *skS, const uint8_t *pkS, const uint8_t *ikmE, uint8_t *enc, uint8_t *ss,
                                    uint8_t *ok, size_t n, int device) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return CIRCL_HIP_OK;
    if (!pkR || !skS || !ikmE || !enc || !ss) return CIRCL_HIP_EPARAM;
    const size_t N = key_bytes(kem), S = ss_bytes(kem);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        std::vector<HIn> ins = {{pkR + lo * N, N}, {skS + lo * N, N, true}, {ikmE + lo * N, N, true}};
        if (pkS) ins.push_back({pkS + lo * N, N});
        return run_pipeline(dev, cnt, ins, {}, {{enc + lo * N, N}, {ss + lo * S, S, true}, {ok ? ok + lo : nullptr, 1}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_hpke_dhkem_auth_encap_dev(kem, c.in[0], c.in[1], pkS ? c.in[3] : nullptr, c.in[2], c.out[0], c.out[1], c.out[2], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

int circl_hip_hpke_dhkem_auth_decap(int kem, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, const uint8_t *pkS, uint8_t *ss, uint8_t *ok,
                                    size_t n, int device) {
    if (!kem_known(kem)) return CIRCL_HIP_EPARAM;
    if (n == 0) return CIRCL_HIP_OK;
    if (!skR || !enc || !pkS || !ss) return CIRCL_HIP_EPARAM;
    const size_t N = key_bytes(kem), S = ss_bytes(kem);
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        std::vector<HIn> ins = {{skR + lo * N, N, true}, {enc + lo * N, N}, {pkS + lo * N, N}};
        if (pkR) ins.push_back({pkR + lo * N, N});
        return run_pipeline(dev, cnt, ins, {}, {{ss + lo * S, S, true}, {ok ? ok + lo : nullptr, 1}}, kNoWs, opts, [&](Chunk &c) {
            return circl_hip_hpke_dhkem_auth_decap_dev(kem, c.in[0], pkR ? c.in[3] : nullptr, c.in[1], c.in[2], c.out[0], c.out[1], c.cnt, c.st);
        });
    }, kHeavyOneDeviceMax);
}

// ---- batch SHA-256 (crypto/sha256.Sum256), the twin of circl_hip_sha512 ------------------------------------------------------
int circl_hip_sha256(const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *out32, size_t n, int device) {
    if (n == 0) return CIRCL_HIP_OK;
    if (!msg_off || !out32) return CIRCL_HIP_EPARAM;
    PipeOpts opts;
    opts.chunk_items = host_chunk_items(size_t(1) << 16);
    return shard(n, device, [&](int dev, size_t lo, size_t cnt) {
        return run_pipeline(dev, cnt, {}, {{msg_blob, msg_off + lo}}, {{out32 + lo * 32, 32}}, kNoWs, opts, [&](Chunk &c) {
            ProfScope ps(CIRCL_HIP_KERNEL_SHA256, c.st);
            hipLaunchKernelGGL(circl::dhkem::sha256_kernel, lanes_grid(c.cnt), dim3(64), 0, c.st, c.blob[0], c.off[0], reinterpret_cast<uint32_t *>(c.out[0]),
                               c.cnt);
            HIP_TRY(hipGetLastError());
            return CIRCL_HIP_OK;
        });
    });
}

}  // extern "C"
