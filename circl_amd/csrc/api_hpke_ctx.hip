// api_hpke_ctx.hip -- batch HPKE contexts (hpke/hpke.go, hpke/util.go, hpke/aead.go; RFC 9180 sections 5 and 6) behind the C ABI
// (include/circl_hip.h): Setup of a sender / a receiver, Seal, Open and Export on context rows, and the single-shot forms, over the
// DHKEMs of api_hpke.hip, HKDF-SHA256 / HKDF-SHA512 and ChaCha20-Poly1305 or the export-only AEAD.  No CPU compute path.
//
// Every entry point fills one Call (the pointers as the ABI passes them: device pointers for a _dev form, host pointers for a
// host form) and goes through check() -- the argument contract, before any device is looked for -- and then launch() or host_pipeline().
// Every host form goes through shard / run_pipeline like the DHKEM's.  Seal, Open and their single-shot forms read and write blobs
// that share ONE offset array: the plaintext side is a blob / a ragged output over pt_off, the ciphertext side the same with a pad
// of 16 bytes per item (host_common.h HBlob / HOut).  Plaintexts and the secret rows are wiped from the page-locked staging, and
// the device staging of every chunk is zeroed whole.
// The arrays a host form stages are declared once each, by the Call field they come from and go back to (host_compose.h Bind).
#include "host_compose.h"
#include "hpke_kernels.h"

using namespace circl::host;
namespace hp = circl::hpke;
using circl::dhkem::X25519;
using circl::dhkem::X448;
using circl::hkdf::Sha256;
using circl::hkdf::Sha512;

namespace {

enum Op { kSetupSender, kSetupReceiver, kSeal, kOpen, kExportRows };

struct Call {
    Op op;
    int kem = 0x20, kdf = 1, aead = 3, mode = 0, what = hp::kStoreContext;
    // setup
    const uint8_t *pkR = nullptr, *ikmE = nullptr, *skR = nullptr, *skS = nullptr, *pkS = nullptr, *enc_in = nullptr;
    uint8_t *enc_out = nullptr;
    const uint8_t *info = nullptr, *psk = nullptr, *psk_id = nullptr;
    const uint64_t *info_off = nullptr, *psk_off = nullptr, *psk_id_off = nullptr;
    // context rows: written by a setup that stores them (stride = context_size), read by Seal / Open / Export
    uint8_t *ctx_out = nullptr;
    const uint8_t *ctx_in = nullptr;
    size_t ctx_stride = 0;
    const uint64_t *seq = nullptr;
    // AEAD: in = plaintext blob (Seal) or ciphertext blob (Open), out = the other one
    const uint8_t *in = nullptr, *aad = nullptr;
    const uint64_t *pt_off = nullptr, *aad_off = nullptr;
    uint8_t *out = nullptr;
    // Export
    const uint8_t *exp = nullptr;
    const uint64_t *exp_off = nullptr;
    size_t L = 0;
    uint8_t *exp_out = nullptr;
    uint8_t *ok = nullptr;
    size_t n = 0;

    bool setup() const { return op == kSetupSender || op == kSetupReceiver; }
    bool sender() const { return op == kSetupSender || op == kSeal; }
    bool does_aead() const { return op == kSeal || op == kOpen || (setup() && what == hp::kAead); }
    bool does_export() const { return op == kExportRows || (setup() && what == hp::kExport); }
};

size_t key_bytes(int kem) { return kem == 0x20 ? 32 : 56; }
size_t hash_bytes(int kdf) { return kdf == 1 ? 32 : kdf == 3 ? 64 : 0; }
size_t ctx_bytes(int kdf) { return hash_bytes(kdf) ? 48 + hash_bytes(kdf) : 0; }

// the argument contract, the same for both forms; nothing here looks for a device
int check(const Call &c) {
    const bool kem_ok = c.kem == 0x20 || c.kem == 0x21, kdf_ok = c.kdf == 1 || c.kdf == 3;
    const bool aead_ok = c.aead == hp::AEAD_CHACHA20POLY1305 || c.aead == hp::AEAD_EXPORT_ONLY;
    if (c.setup() || c.does_export()) {
        if (!kem_ok || !kdf_ok || !aead_ok) return CIRCL_HIP_EPARAM;
    }
    if (c.does_aead() && c.aead != hp::AEAD_CHACHA20POLY1305) return CIRCL_HIP_EPARAM;  // export-only has no Seal / Open
    if (c.setup() && (c.mode < 0 || c.mode > 3)) return CIRCL_HIP_EPARAM;
    if (c.does_export() && (c.L == 0 || c.L > 255 * hash_bytes(c.kdf))) return CIRCL_HIP_EPARAM;
    if (!c.setup()) {
        if (c.ctx_stride % 4 || c.ctx_stride < (c.op == kExportRows ? ctx_bytes(c.kdf) : size_t(48))) return CIRCL_HIP_EPARAM;
    }
    if (c.n == 0) return CIRCL_HIP_OK;
    if (c.setup()) {
        const bool auth = c.mode & 2, with_psk = c.mode & 1;
        if (!with_psk && (c.psk || c.psk_id)) return CIRCL_HIP_EPARAM;
        if (c.op == kSetupSender) {
            if (!c.pkR || !c.ikmE || !c.enc_out) return CIRCL_HIP_EPARAM;
            if (auth ? (!c.skS || !c.pkS) : (c.skS || c.pkS)) return CIRCL_HIP_EPARAM;
        } else {
            if (!c.skR || !c.enc_in) return CIRCL_HIP_EPARAM;
            if (auth ? !c.pkS : c.pkS != nullptr) return CIRCL_HIP_EPARAM;
        }
        if ((c.info && !c.info_off) || (c.psk && !c.psk_off) || (c.psk_id && !c.psk_id_off)) return CIRCL_HIP_EPARAM;
        if (c.what == hp::kStoreContext && !c.ctx_out) return CIRCL_HIP_EPARAM;
    } else if (!c.ctx_in) {
        return CIRCL_HIP_EPARAM;
    }
    if (c.does_aead()) {
        // a NULL plaintext blob with offsets means empty plaintexts; a ciphertext always has its tags
        if (!c.out || (c.aad && !c.aad_off)) return CIRCL_HIP_EPARAM;
        if (c.sender() ? (c.in && !c.pt_off) : !c.in) return CIRCL_HIP_EPARAM;
    }
    if (c.does_export() && (!c.exp_out || (c.exp && !c.exp_off))) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

const uint32_t *w(const uint8_t *p) { return reinterpret_cast<const uint32_t *>(p); }
uint32_t *w(uint8_t *p) { return reinterpret_cast<uint32_t *>(p); }

// one launch on device pointers
int launch(const Call &c, hipStream_t st) {
    if (!aligned<4>(c.pkR, c.ikmE, c.skR, c.skS, c.pkS, c.enc_in, c.enc_out, c.ctx_in, c.ctx_out) ||
        !aligned<8>(c.info_off, c.psk_off, c.psk_id_off, c.pt_off, c.aad_off, c.exp_off, c.seq))
        return CIRCL_HIP_EWORKSPACE;
    if (ndev() <= 0) return CIRCL_HIP_ENODEV;
    const dim3 grid = lanes_grid(c.n), block(64);
    if (c.setup()) {
        hp::SetupArgs a = {};
        a.pkR = w(c.pkR); a.ikmE = w(c.ikmE); a.skR = w(c.skR); a.skS = w(c.skS); a.pkS = w(c.pkS);
        a.enc_out = w(c.enc_out); a.enc_in = w(c.enc_in);
        a.info = c.info; a.psk = c.psk; a.psk_id = c.psk_id;
        a.info_off = c.info_off; a.psk_off = c.psk_off; a.psk_id_off = c.psk_id_off;
        a.ok = c.ok;
        a.kem = c.kem; a.kdf = c.kdf; a.aead = c.aead; a.mode = c.mode; a.what = c.what;
        a.ctx = w(c.ctx_out); a.ctx_stride_words = ctx_bytes(c.kdf) / 4;
        // a Seal without a plaintext blob: every plaintext is empty and the offsets are not read
        a.in = c.in; a.aad = c.aad; a.pt_off = c.in ? c.pt_off : nullptr; a.aad_off = c.aad_off; a.out = c.out;
        a.exp = c.exp; a.exp_off = c.exp_off; a.L = (uint32_t)c.L; a.exp_out = c.exp_out;
        a.n = c.n;
        ProfScope ps(CIRCL_HIP_KERNEL_HPKE_SETUP, st);
        const bool snd = c.op == kSetupSender, s256 = c.kdf == 1;
#define SETUP_LAUNCH(C, HK)                                                                                      \
    do {                                                                                                         \
        if (snd) hipLaunchKernelGGL((hp::setup_kernel<C, HK, true>), grid, block, 0, st, a);                     \
        else hipLaunchKernelGGL((hp::setup_kernel<C, HK, false>), grid, block, 0, st, a);                        \
    } while (0)
        if (c.kem == 0x20 && s256) SETUP_LAUNCH(X25519, Sha256);
        else if (c.kem == 0x20) SETUP_LAUNCH(X25519, Sha512);
        else if (s256) SETUP_LAUNCH(X448, Sha256);
        else SETUP_LAUNCH(X448, Sha512);
#undef SETUP_LAUNCH
    } else if (c.op == kExportRows) {
        const hp::ExportArgs a = {w(c.ctx_in), c.ctx_stride / 4, c.kem, c.kdf, c.aead, c.exp, c.exp_off, (uint32_t)c.L, c.exp_out, c.n};
        ProfScope ps(CIRCL_HIP_KERNEL_HPKE_EXPORT, st);
        if (c.kdf == 1) hipLaunchKernelGGL(hp::export_kernel<Sha256>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(hp::export_kernel<Sha512>, grid, block, 0, st, a);
    } else {
        const hp::AeadArgs a = {w(c.ctx_in), c.ctx_stride / 4, c.seq, c.in, c.aad, c.in ? c.pt_off : nullptr, c.aad_off, c.out, c.ok, c.n};
        ProfScope ps(CIRCL_HIP_KERNEL_HPKE_AEAD, st);
        if (c.op == kSeal) hipLaunchKernelGGL(hp::aead_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(hp::aead_kernel<false>, grid, block, 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return CIRCL_HIP_OK;
}

// ---- host forms: shard / run_pipeline -------------------------------------------------------------------------------------------
int host_pipeline(const Call &c, int device) {
    const size_t N = key_bytes(c.kem), CS = c.setup() ? ctx_bytes(c.kdf) : c.ctx_stride;
    const PipeOpts opts = secret_opts(size_t(1) << 16);
    // the offsets that size both AEAD blobs, as launch() reads them; without them every plaintext is empty and a ciphertext is a row of 16
    const uint64_t *pt_off = c.does_aead() && c.in ? c.pt_off : nullptr;
    const bool sealing = c.does_aead() && c.sender(), opening = c.does_aead() && !c.sender();  // plaintext in / plaintext out: the secret side
    return shard(c.n, device, [&](int dev, size_t lo, size_t cnt) {
        Bind<Call> b(c, lo);
        b.rows(&Call::pkR, N, false);
        b.rows(&Call::ikmE, N, true);
        b.rows(&Call::skR, N, true);
        b.rows(&Call::skS, N, true);
        b.rows(&Call::pkS, N, false);
        b.rows(&Call::enc_in, N, false);
        b.rows(&Call::ctx_in, CS, true);
        b.rows(&Call::seq, 8, false);
        b.blob(&Call::info, &Call::info_off, false);
        b.blob(&Call::psk, &Call::psk_off, true);
        b.blob(&Call::psk_id, &Call::psk_id_off, false);
        b.blob(&Call::exp, &Call::exp_off, false);
        b.blob(&Call::aad, &Call::aad_off, false);
        b.blob(&Call::in, &Call::pt_off, sealing, sealing ? 0 : 16, pt_off != nullptr);
        if (!pt_off) b.rows(&Call::in, 16, false, false, opening);   // an Open of empty plaintexts reads rows of tags
        b.out(&Call::enc_out, N, false, c.op == kSetupSender);
        b.out(&Call::ctx_out, CS, true, c.setup() && c.what == hp::kStoreContext);
        b.out(&Call::exp_out, c.L, true, c.does_export());
        b.out(&Call::ok, 1, false, c.setup() || c.op == kOpen);
        if (pt_off) b.ragged(&Call::out, &Call::pt_off, opening, sealing ? 16 : 0);
        else b.out(&Call::out, sealing ? 16 : 0, false, c.does_aead());
        return run_pipeline(dev, cnt, b.ins, b.blobs, b.outs, kNoWs, opts, [&](Chunk &k) { return launch(b.on(k), k.st); });
    }, kHeavyOneDeviceMax);
}

Call sender_call(int kem, int kdf, int aead, int mode, const uint8_t *pkR, const uint8_t *ikmE, const uint8_t *skS, const uint8_t *pkS, const uint8_t *info_blob,
                 const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off, uint8_t *enc,
                 uint8_t *ok, size_t n) {
    Call c;
    c.op = kSetupSender; c.kem = kem; c.kdf = kdf; c.aead = aead; c.mode = mode;
    c.pkR = pkR; c.ikmE = ikmE; c.skS = skS; c.pkS = pkS; c.enc_out = enc;
    c.info = info_blob; c.info_off = info_off; c.psk = psk_blob; c.psk_off = psk_off; c.psk_id = psk_id_blob; c.psk_id_off = psk_id_off;
    c.ok = ok; c.n = n;
    return c;
}

Call receiver_call(int kem, int kdf, int aead, int mode, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, const uint8_t *pkS, const uint8_t *info_blob,
                   const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off, uint8_t *ok,
                   size_t n) {
    Call c;
    c.op = kSetupReceiver; c.kem = kem; c.kdf = kdf; c.aead = aead; c.mode = mode;
    c.skR = skR; c.pkR = pkR; c.enc_in = enc; c.pkS = pkS;
    c.info = info_blob; c.info_off = info_off; c.psk = psk_blob; c.psk_off = psk_off; c.psk_id = psk_id_blob; c.psk_id_off = psk_id_off;
    c.ok = ok; c.n = n;
    return c;
}

void with_aead(Call &c, const uint8_t *in, const uint64_t *pt_off, const uint8_t *aad, const uint64_t *aad_off, uint8_t *out) {
    c.what = hp::kAead; c.in = in; c.pt_off = pt_off; c.aad = aad; c.aad_off = aad_off; c.out = out;
}
void with_export(Call &c, const uint8_t *exp, const uint64_t *exp_off, size_t L, uint8_t *out) {
    c.what = hp::kExport; c.exp = exp; c.exp_off = exp_off; c.L = L; c.exp_out = out;
}
Call rows_call(Op op, int aead, const uint8_t *ctx, size_t ctx_stride, size_t n) {
    Call c;
    c.op = op; c.aead = aead; c.ctx_in = ctx; c.ctx_stride = ctx_stride; c.n = n;
    return c;
}

}  // namespace

// the setup arguments of a sender / a receiver as every entry point spells them
#define SENDER_PARAMS                                                                                                                                       \
    int kem, int kdf, int aead, int mode, const uint8_t *pkR, const uint8_t *ikmE, const uint8_t *skS, const uint8_t *pkS, const uint8_t *info_blob,        \
        const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off
#define SENDER_ARGS kem, kdf, aead, mode, pkR, ikmE, skS, pkS, info_blob, info_off, psk_blob, psk_off, psk_id_blob, psk_id_off
#define RECEIVER_PARAMS                                                                                                                                     \
    int kem, int kdf, int aead, int mode, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, const uint8_t *pkS, const uint8_t *info_blob,         \
        const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off
#define RECEIVER_ARGS kem, kdf, aead, mode, skR, pkR, enc, pkS, info_blob, info_off, psk_blob, psk_off, psk_id_blob, psk_id_off

extern "C" {

size_t circl_hip_hpke_context_size(int kdf) { return ctx_bytes(kdf); }

BOTH_FORMS(circl_hip_hpke_setup_sender, P(SENDER_PARAMS, uint8_t *enc, uint8_t *ctx, uint8_t *ok), {
    Call c = sender_call(SENDER_ARGS, enc, ok, n);
    c.ctx_out = ctx;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_hpke_setup_receiver, P(RECEIVER_PARAMS, uint8_t *ctx, uint8_t *ok), {
    Call c = receiver_call(RECEIVER_ARGS, ok, n);
    c.ctx_out = ctx;
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_hpke_seal,
           P(int aead, const uint8_t *ctx, size_t ctx_stride, const uint64_t *seq, const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob,
             const uint64_t *aad_off, uint8_t *ct_blob),
           {
               Call c = rows_call(kSeal, aead, ctx, ctx_stride, n);
               c.seq = seq;
               with_aead(c, pt_blob, pt_off, aad_blob, aad_off, ct_blob);
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_hpke_open,
           P(int aead, const uint8_t *ctx, size_t ctx_stride, const uint64_t *seq, const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob,
             const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok),
           {
               Call c = rows_call(kOpen, aead, ctx, ctx_stride, n);
               c.seq = seq;
               c.ok = ok;
               with_aead(c, ct_blob, pt_off, aad_blob, aad_off, pt_blob);
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_hpke_export,
           P(int kdf, int kem, int aead, const uint8_t *ctx, size_t ctx_stride, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out), {
               Call c = rows_call(kExportRows, aead, ctx, ctx_stride, n);
               c.kem = kem;
               c.kdf = kdf;
               with_export(c, exp_blob, exp_off, L, out);
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_hpke_seal_single,
           P(SENDER_PARAMS, const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *enc, uint8_t *ct_blob,
             uint8_t *ok),
           {
               Call c = sender_call(SENDER_ARGS, enc, ok, n);
               with_aead(c, pt_blob, pt_off, aad_blob, aad_off, ct_blob);
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_hpke_open_single,
           P(RECEIVER_PARAMS, const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok), {
               Call c = receiver_call(RECEIVER_ARGS, ok, n);
               with_aead(c, ct_blob, pt_off, aad_blob, aad_off, pt_blob);
               return run_call(c, dev_, device, stream);
           })

BOTH_FORMS(circl_hip_hpke_export_single, P(SENDER_PARAMS, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *enc, uint8_t *out, uint8_t *ok), {
    Call c = sender_call(SENDER_ARGS, enc, ok, n);
    with_export(c, exp_blob, exp_off, L, out);
    return run_call(c, dev_, device, stream);
})

BOTH_FORMS(circl_hip_hpke_export_single_receiver, P(RECEIVER_PARAMS, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out, uint8_t *ok), {
    Call c = receiver_call(RECEIVER_ARGS, ok, n);
    with_export(c, exp_blob, exp_off, L, out);
    return run_call(c, dev_, device, stream);
})

}  // extern "C"
