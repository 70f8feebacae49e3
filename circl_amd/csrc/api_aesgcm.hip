// api_aesgcm.hip -- the batch AEADs AES-128-GCM and AES-256-GCM (hpke/aead.go's AEAD ids 1 and 2; NIST SP 800-38D) behind the C ABI
// (include/circl_hip.h): Seal and Open over ragged batches, one item per lane.  No CPU compute path.
//
// Both entry points fill one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a host
// form) and go through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// The host forms go through shard / run_pipeline as Ascon's and HPKE's Seal / Open do: the plaintext side is a blob / a ragged output
// over pt_off, the ciphertext side the same with a pad of 16 bytes per item (host_common.h HBlob / HOut).  Keys and plaintexts are
// wiped from the page-locked staging, and the device staging of every chunk is zeroed whole.  A key or a base nonce shared by the
// batch (stride 0) is a per-call input: one row is staged with every chunk.  Nonce rows further than 12 bytes apart are gathered
// first (they are public), so that a host form reads 12 bytes of a row and nothing behind the last one.  These calls do not join
// coalesced batches.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
#include "aesgcm_kernels.h"
#include "host_compose.h"

#include <cstring>
#include <vector>

using namespace circl::host;
namespace ag = circl::aesgcm;

namespace {

struct Call {
    bool seal = true;
    int key_bytes = 0;
    const uint8_t *key = nullptr, *nonce = nullptr;
    size_t key_stride = 0, nonce_stride = 0;
    const uint64_t *seq = nullptr;
    // in = plaintext blob (Seal) or ciphertext blob (Open), out = the other one
    const uint8_t *in = nullptr, *aad = nullptr;
    const uint64_t *pt_off = nullptr, *aad_off = nullptr;
    uint8_t *out = nullptr, *ok = nullptr;
    size_t n = 0;
    bool host = false;   // a host form: the offsets can be read
};

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    if (!ag::key_bytes_ok(c.key_bytes)) return CIRCL_HIP_EPARAM;
    if (c.key_stride != 0 && (c.key_stride % 4 || c.key_stride < (size_t)c.key_bytes)) return CIRCL_HIP_EPARAM;
    if (c.nonce_stride == 0 ? !c.seq : (c.nonce_stride % 4 || c.nonce_stride < (size_t)ag::NONCE_BYTES)) return CIRCL_HIP_EPARAM;
    if (c.n == 0) return CIRCL_HIP_OK;
    if (!c.key || !c.nonce || !c.out || (c.aad && !c.aad_off)) return CIRCL_HIP_EPARAM;
    // a NULL plaintext blob means empty plaintexts; a ciphertext always has its tags
    if (c.seal ? (c.in && !c.pt_off) : !c.in) return CIRCL_HIP_EPARAM;
    if (c.host && c.pt_off && (c.in || !c.seal)) {   // SP 800-38D 5.2.1.1: a plaintext has at most 2^39 - 256 bits
        for (size_t i = 0; i < c.n; i++)
            if (c.pt_off[i + 1] < c.pt_off[i] || c.pt_off[i + 1] - c.pt_off[i] > ag::MAX_PT_BYTES) return CIRCL_HIP_EPARAM;
    }
    return CIRCL_HIP_OK;
}

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }

// one launch on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.key, c.nonce) || !aligned<8>(c.pt_off, c.aad_off, c.seq)) return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    // a Seal without a plaintext blob: every plaintext is empty and the offsets are not read
    const ag::Args a = {w(c.key), c.key_stride / 4, w(c.nonce), c.nonce_stride / 4, c.seq, c.in, c.aad, c.in ? c.pt_off : nullptr, c.aad_off, c.out, c.ok, c.n};
    const dim3 grid = lanes_grid(c.n), block(64);
    ProfScope ps(c.seal ? CIRCL_HIP_KERNEL_AESGCM_SEAL : CIRCL_HIP_KERNEL_AESGCM_OPEN, st);
#define AESGCM_LAUNCH(KB)                                                                     \
    do {                                                                                      \
        if (c.seal) hipLaunchKernelGGL((ag::kernel<KB, true>), grid, block, 0, st, a);        \
        else hipLaunchKernelGGL((ag::kernel<KB, false>), grid, block, 0, st, a);              \
    } while (0)
    if (c.key_bytes == ag::AES128GCM) AESGCM_LAUNCH(ag::AES128GCM);
    else AESGCM_LAUNCH(ag::AES256GCM);
#undef AESGCM_LAUNCH
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int host_pipeline(const Call &caller, int device) {
    Call c = caller;
    // nonce rows further apart than their 12 bytes: gathered, so that nothing behind a row's nonce is read or staged
    std::vector<uint8_t> packed;
    if (c.nonce_stride > (size_t)ag::NONCE_BYTES) {
        packed.resize(c.n * ag::NONCE_BYTES);
        for (size_t i = 0; i < c.n; i++) memcpy(&packed[i * ag::NONCE_BYTES], c.nonce + i * c.nonce_stride, ag::NONCE_BYTES);
        c.nonce = packed.data();
        c.nonce_stride = ag::NONCE_BYTES;
    }
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    const bool shared = c.key_stride == 0, one_nonce = c.nonce_stride == 0;
    // the offsets that size both blobs, as launch() reads them; without them every plaintext is empty and a ciphertext is a row of 16
    const uint64_t *pt_off = c.in ? c.pt_off : nullptr;
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        b.rows(&Call::key, shared ? (size_t)c.key_bytes : c.key_stride, true, shared);
        b.rows(&Call::nonce, ag::NONCE_BYTES, false, one_nonce);
        b.rows(&Call::seq, 8, false);
        b.blob(&Call::aad, &Call::aad_off, false);
        b.blob(&Call::in, &Call::pt_off, c.seal, c.seal ? 0 : 16, pt_off != nullptr);   // plaintext in (Seal): the secret side
        if (!pt_off) b.rows(&Call::in, 16, false, false, !c.seal);                      // an Open of empty plaintexts reads rows of tags
        if (pt_off) b.ragged(&Call::out, &Call::pt_off, !c.seal, c.seal ? 16 : 0);
        else b.out(&Call::out, c.seal ? 16 : 0, false);
        b.out(&Call::ok, 1, false, !c.seal);
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

int run(Call &c, bool dev, int device, void *stream) {
    c.host = !dev;
    return run_call(c, dev, device, stream);
}

}  // namespace

extern "C" {

BOTH_FORMS(circl_hip_aesgcm_seal,
           P(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq, const uint8_t *pt_blob,
             const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *ct_blob),
           {
               Call c;
               c.seal = true; c.key_bytes = key_bytes; c.key = key; c.key_stride = key_stride; c.nonce = nonce12; c.nonce_stride = nonce_stride; c.seq = seq;
               c.in = pt_blob; c.pt_off = pt_off; c.aad = aad_blob; c.aad_off = aad_off; c.out = ct_blob; c.n = n;
               return run(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_aesgcm_open,
           P(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq, const uint8_t *ct_blob,
             const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok),
           {
               Call c;
               c.seal = false; c.key_bytes = key_bytes; c.key = key; c.key_stride = key_stride; c.nonce = nonce12; c.nonce_stride = nonce_stride; c.seq = seq;
               c.in = ct_blob; c.pt_off = pt_off; c.aad = aad_blob; c.aad_off = aad_off; c.out = pt_blob; c.ok = ok; c.n = n;
               return run(c, dev_, device, stream);
           })

}  // extern "C"
