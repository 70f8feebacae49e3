// circl/ed448.hpp -- host-side mirror of cloudflare/circl's sign.Scheme for "Ed448" and "Ed448-Dilithium3" on the HIP batch
// engine (sign/ed448/signapi.go, sign/eddilithium3/signapi.go).  Same conventions as circl/ed25519.hpp:
//
//   Scheme.Name / PublicKeySize / PrivateKeySize / SignatureSize / SeedSize     same names and sizes
//   SupportsContext()                              true for "Ed448": Sign / Verify take the context from the options
//                                                  (ErrContextTooLong over 255 bytes when signing, false when verifying);
//                                                  false for "Ed448-Dilithium3": a non-empty context throws ErrContextNotSupported
//   UnmarshalBinaryPublicKey / PrivateKey          length checks (ErrPubKeySize / ErrPrivKeySize)
//   DeriveKey(seed)                                throws std::invalid_argument on a bad seed length
//   Sign / Verify                                  ErrTypeMismatch for a key of another scheme; Verify is false for a
//                                                  signature of the wrong length
//   DeriveKeyBatch / SignBatch / VerifyBatch       the batch calls: one key per item; contexts as a second blob (Ed448 only,
//                                                  NULL: every context empty)
// Ed448ph (SignPh / VerifyPh) is not provided.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../circl_hip.h"
#include "sign.hpp"

namespace circl {
namespace ed448 {

using sign::Bytes;
using sign::SignatureOpts;

class Scheme;
struct PublicKey {
    const Scheme *scheme = nullptr;
    Bytes packed;
    Bytes MarshalBinary() const { return packed; }
};
struct PrivateKey {
    const Scheme *scheme = nullptr;
    Bytes packed;
    Bytes MarshalBinary() const { return packed; }
};

class Scheme {
  public:
    // dilithium = false: "Ed448"; true: "Ed448-Dilithium3"
    explicit Scheme(bool dilithium) : ed_dil_(dilithium) {}
    std::string Name() const { return ed_dil_ ? "Ed448-Dilithium3" : "Ed448"; }
    int PublicKeySize() const { return ed_dil_ ? 2009 : 57; }
    int PrivateKeySize() const { return ed_dil_ ? 4057 : 114; }
    int SignatureSize() const { return ed_dil_ ? 3407 : 114; }
    int SeedSize() const { return 57; }
    bool SupportsContext() const { return !ed_dil_; }
    int device = 0;

    PublicKey UnmarshalBinaryPublicKey(const Bytes &buf) const {
        if ((int)buf.size() != PublicKeySize()) throw sign::ErrPubKeySize();
        return PublicKey{this, buf};
    }
    PrivateKey UnmarshalBinaryPrivateKey(const Bytes &buf) const {
        if ((int)buf.size() != PrivateKeySize()) throw sign::ErrPrivKeySize();
        return PrivateKey{this, buf};
    }
    std::pair<PublicKey, PrivateKey> DeriveKey(const Bytes &seed) const {
        if ((int)seed.size() != SeedSize()) throw std::invalid_argument("seed must be of length SeedSize");
        Bytes pk, sk;
        DeriveKeyBatch(seed.data(), 1, pk, sk);
        return {PublicKey{this, pk}, PrivateKey{this, sk}};
    }
    Bytes Sign(const PrivateKey &sk, const Bytes &msg, const SignatureOpts *opts = nullptr) const {
        if (sk.scheme != this) throw sign::ErrTypeMismatch();
        const std::string ctx = opts ? opts->Context : std::string();
        if (!SupportsContext() && !ctx.empty()) throw sign::ErrContextNotSupported();
        if (ctx.size() > 255) throw sign::ErrContextTooLong();
        const uint64_t off[2] = {0, msg.size()}, coff[2] = {0, ctx.size()};
        const uint8_t pad = 0;
        Bytes sig(SignatureSize());
        SignBatch(sk.packed.data(), msg.empty() ? &pad : msg.data(), off, ctx.empty() ? nullptr : reinterpret_cast<const uint8_t *>(ctx.data()), coff, 1,
                  sig.data());
        return sig;
    }
    bool Verify(const PublicKey &pk, const Bytes &msg, const Bytes &sig, const SignatureOpts *opts = nullptr) const {
        if (pk.scheme != this) throw sign::ErrTypeMismatch();
        const std::string ctx = opts ? opts->Context : std::string();
        if (!SupportsContext() && !ctx.empty()) throw sign::ErrContextNotSupported();
        if ((int)sig.size() != SignatureSize() || ctx.size() > 255) return false;
        const uint64_t off[2] = {0, msg.size()}, coff[2] = {0, ctx.size()};
        const uint8_t pad = 0;
        uint8_t ok = 0;
        VerifyBatch(pk.packed.data(), sig.data(), msg.empty() ? &pad : msg.data(), off, ctx.empty() ? nullptr : reinterpret_cast<const uint8_t *>(ctx.data()),
                    coff, 1, &ok);
        return ok != 0;
    }

    // batches: seeds[n][57] -> pk[n][PublicKeySize], sk[n][PrivateKeySize]; messages (and, for Ed448, contexts) as a blob + n + 1
    // offsets; ctx_blob == nullptr: every context empty (the only form "Ed448-Dilithium3" takes)
    void DeriveKeyBatch(const uint8_t *seeds, size_t n, Bytes &pk, Bytes &sk) const {
        pk.assign(n * PublicKeySize(), 0);
        sk.assign(n * PrivateKeySize(), 0);
        if (!n) return;
        check(ed_dil_ ? circl_hip_eddilithium3_keygen(seeds, pk.data(), sk.data(), n, device) : circl_hip_ed448_keygen(seeds, pk.data(), sk.data(), n, device));
    }
    void SignBatch(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off, size_t n,
                   uint8_t *sig) const {
        if (ed_dil_ && ctx_blob) throw sign::ErrContextNotSupported();
        const int rc = ed_dil_ ? circl_hip_eddilithium3_sign(sk, msg_blob, msg_off, sig, n, device)
                               : circl_hip_ed448_sign(sk, msg_blob, msg_off, ctx_blob, ctx_off, sig, n, device);
        if (!ed_dil_ && rc == CIRCL_HIP_EPARAM && ctx_blob) throw sign::ErrContextTooLong();
        check(rc);
    }
    void VerifyBatch(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off,
                     size_t n, uint8_t *ok) const {
        if (ed_dil_ && ctx_blob) throw sign::ErrContextNotSupported();
        check(ed_dil_ ? circl_hip_eddilithium3_verify(pk, sig, msg_blob, msg_off, ok, n, device)
                      : circl_hip_ed448_verify(pk, sig, msg_blob, msg_off, ctx_blob, ctx_off, ok, n, device));
    }

  private:
    bool ed_dil_;
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw sign::ErrDevice(std::string("circl-hip: error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
};

// sign/schemes.ByName("Ed448") / ("Ed448-Dilithium3")
inline const Scheme &ByName(const std::string &name) {
    static const Scheme ed(false), eddil(true);
    if (name == "Ed448") return ed;
    if (name == "Ed448-Dilithium3") return eddil;
    throw std::invalid_argument("unknown scheme " + name);
}

}  // namespace ed448
}  // namespace circl
