// api_ascon.hip -- the batch Ascon AEADs Ascon128, Ascon128a and Ascon80pq (cipher/ascon/ascon.go) behind the C ABI
// (include/circl_hip.h): Seal and Open over ragged batches, one item per lane.  No CPU compute path.
//
// Both entry points fill one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a host
// form) and go through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// The host forms go through shard / run_pipeline as HPKE's Seal / Open do: the plaintext side is a blob / a ragged output over pt_off,
// the ciphertext side the same with a pad of 16 bytes per item (host_common.h HBlob / HOut).  Keys and plaintexts are wiped from the
// page-locked staging, and the device staging of every chunk is zeroed whole.  A key shared by the batch (stride 0) is a per-call input:
// one row is staged with every chunk.  These calls do not join coalesced batches.
#include "ascon_kernels.h"
#include "host_compose.h"

using namespace circl::host;
namespace as = circl::ascon;

namespace {

struct Call {
    bool seal = true;
    int mode = 0;
    const uint8_t *key = nullptr, *nonce = nullptr;
    size_t key_stride = 0;
    // in = plaintext blob (Seal) or ciphertext blob (Open), out = the other one
    const uint8_t *in = nullptr, *aad = nullptr;
    const uint64_t *pt_off = nullptr, *aad_off = nullptr;
    uint8_t *out = nullptr, *ok = nullptr;
    size_t n = 0;
};

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (!as::mode_ok(c.mode)) return CIRCL_HIP_EPARAM;
    if (c.key_stride != 0 && (c.key_stride % 4 || c.key_stride < (size_t)as::key_bytes(c.mode))) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.key || !c.nonce || !c.out || (c.aad && !c.aad_off)) return CIRCL_HIP_EPARAM;
    // a NULL plaintext blob means empty plaintexts; a ciphertext always has its tags
    if (c.seal ? (c.in && !c.pt_off) : !c.in) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }

// one launch on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.key, c.nonce) || !aligned<8>(c.pt_off, c.aad_off)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    // a Seal without a plaintext blob: every plaintext is empty and the offsets are not read
    const as::Args a = {w(c.key), c.key_stride / 4, w(c.nonce), c.in, c.aad, c.in ? c.pt_off : nullptr, c.aad_off, c.out, c.ok, c.n};
    const dim3 grid = lanes_grid(c.n), block(64);
    ProfScope ps(c.seal ? CIRCL_HIP_KERNEL_ASCON_SEAL : CIRCL_HIP_KERNEL_ASCON_OPEN, st);
#define ASCON_LAUNCH(MODE)                                                                      \
    do {                                                                                        \
        if (c.seal) hipLaunchKernelGGL((as::kernel<MODE, true>), grid, block, 0, st, a);        \
        else hipLaunchKernelGGL((as::kernel<MODE, false>), grid, block, 0, st, a);              \
    } while (0)
    if (c.mode == as::ASCON128) ASCON_LAUNCH(as::ASCON128);
    else if (c.mode == as::ASCON128A) ASCON_LAUNCH(as::ASCON128A);
    else ASCON_LAUNCH(as::ASCON80PQ);
#undef ASCON_LAUNCH
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const bool shared = c.key_stride == 0;
    const size_t key_row = shared ? (size_t)as::key_bytes(c.mode) : c.key_stride;
    // the offsets that size both blobs, as launch() reads them; without them every plaintext is empty and a ciphertext is a row of 16
    const uint64_t *pt_off = c.in ? c.pt_off : nullptr;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        std::vector<HIn> ins;
        std::vector<HBlob> blobs;
        std::vector<HOut> outs;
        HIn key = {c.key + (shared ? 0 : lo * key_row), key_row, true};
        key.per_call = shared;
        ins.push_back(key);                                            // 0
        ins.push_back({c.nonce + lo * 16, 16, false});                 // 1
        if (!c.seal && !pt_off) ins.push_back({c.in + lo * 16, 16, false});  // 2: an Open of empty plaintexts reads rows of tags
        int b_aad = -1, b_in = -1;
        if (c.aad) {
            blobs.push_back({c.aad, c.aad_off + lo, false});
            b_aad = (int)blobs.size() - 1;
        }
        if (pt_off) {  // plaintext in (Seal): the secret side
            blobs.push_back({c.in + (c.seal ? 0 : 16 * lo), pt_off + lo, c.seal, c.seal ? size_t(0) : size_t(16)});
            b_in = (int)blobs.size() - 1;
        }
        if (pt_off) outs.push_back({c.out + (c.seal ? 16 * lo : 0), 0, !c.seal, pt_off + lo, c.seal ? size_t(16) : size_t(0)});
        else outs.push_back({c.seal ? c.out + 16 * lo : c.out, c.seal ? size_t(16) : size_t(0), false});
        if (!c.seal) outs.push_back({c.ok ? c.ok + lo : nullptr, 1, false});
        return run_pipeline(dev, cnt, ins, blobs, outs, kNoWs, opts, [&](Chunk &k) {
            Call d = c;
            d.key = k.in[0]; d.nonce = k.in[1];
            d.aad = b_aad < 0 ? nullptr : k.blob[b_aad]; d.aad_off = b_aad < 0 ? nullptr : k.off[b_aad];
            d.in = b_in < 0 ? (c.seal ? nullptr : k.in[2]) : k.blob[b_in]; d.pt_off = b_in < 0 ? nullptr : k.off[b_in];
            d.out = k.out[0];
            d.ok = c.seal ? nullptr : k.out[1];
            d.n = k.cnt;
            return launch(d, k.st);
        });
    }, kHeavyOneDeviceMax);
}

int run(const Call &c, bool dev, int device, void *stream) {
    if (int rc = check(c)) return rc;
    if (c.n == 0) return CIRCL_HIP_OK;
    return dev ? launch(c, static_cast<hipStream_t>(stream)) : host_pipeline(c, device);
}

}  // namespace

// both forms of one entry point: NAME(params..., n, int device) and NAME_dev(params..., n, void *stream)
#define BOTH_FORMS(NAME, PARAMS, BODY)                                        \
    int NAME(PARAMS, size_t n, int device) {                                  \
        const bool dev_ = false;                                              \
        void *stream = nullptr;                                               \
        BODY                                                                  \
    }                                                                         \
    int NAME##_dev(PARAMS, size_t n, void *stream) {                          \
        const bool dev_ = true;                                               \
        const int device = 0;                                                 \
        BODY                                                                  \
    }
#define P(...) __VA_ARGS__

extern "C" {

size_t circl_hip_ascon_key_size(int mode) { return (size_t)as::key_bytes(mode); }

BOTH_FORMS(circl_hip_ascon_seal,
           P(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob,
             const uint64_t *aad_off, uint8_t *ct_blob),
           {
               Call c;
               c.seal = true; c.mode = mode; c.key = key; c.key_stride = key_stride; c.nonce = nonce16;
               c.in = pt_blob; c.pt_off = pt_off; c.aad = aad_blob; c.aad_off = aad_off; c.out = ct_blob; c.n = n;
               return run(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_ascon_open,
           P(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob,
             const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok),
           {
               Call c;
               c.seal = false; c.mode = mode; c.key = key; c.key_stride = key_stride; c.nonce = nonce16;
               c.in = ct_blob; c.pt_off = pt_off; c.aad = aad_blob; c.aad_off = aad_off; c.out = pt_blob; c.ok = ok; c.n = n;
               return run(c, dev_, device, stream);
           })

}  // extern "C"
