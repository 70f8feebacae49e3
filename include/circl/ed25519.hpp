// circl/ed25519.hpp -- host-side mirror of cloudflare/circl's sign.Scheme for "Ed25519" and "Ed25519-Dilithium2" on the HIP batch
// engine (sign/ed25519/signapi.go, sign/eddilithium2/signapi.go).  Same conventions as circl/sign.hpp:
//
//   Scheme.Name / PublicKeySize / PrivateKeySize / SignatureSize / SeedSize     same names and sizes
//   SupportsContext() false; a non-empty context throws ErrContextNotSupported (signapi.go: Sign / Verify)
//   UnmarshalBinaryPublicKey / PrivateKey          length checks (ErrPubKeySize / ErrPrivKeySize)
//   DeriveKey(seed)                                throws std::invalid_argument on a bad seed length
//   Sign / Verify                                  ErrTypeMismatch for a key of another scheme; Verify is false for a
//                                                  signature of the wrong length
//   DeriveKeyBatch / SignBatch / VerifyBatch       the batch calls: one key per item
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../circl_hip.h"
#include "sign.hpp"

namespace circl {
namespace ed25519 {

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
    // dilithium = false: "Ed25519"; true: "Ed25519-Dilithium2"
    explicit Scheme(bool dilithium) : ed_dil_(dilithium) {}
    std::string Name() const { return ed_dil_ ? "Ed25519-Dilithium2" : "Ed25519"; }
    int PublicKeySize() const { return ed_dil_ ? 1344 : 32; }
    int PrivateKeySize() const { return ed_dil_ ? 2560 : 64; }
    int SignatureSize() const { return ed_dil_ ? 2484 : 64; }
    int SeedSize() const { return 32; }
    bool SupportsContext() const { return false; }
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
        if (opts && !opts->Context.empty()) throw sign::ErrContextNotSupported();
        const uint64_t off[2] = {0, msg.size()};
        const uint8_t pad = 0;
        Bytes sig(SignatureSize());
        SignBatch(sk.packed.data(), msg.empty() ? &pad : msg.data(), off, 1, sig.data());
        return sig;
    }
    bool Verify(const PublicKey &pk, const Bytes &msg, const Bytes &sig, const SignatureOpts *opts = nullptr) const {
        if (pk.scheme != this) throw sign::ErrTypeMismatch();
        if (opts && !opts->Context.empty()) throw sign::ErrContextNotSupported();
        if ((int)sig.size() != SignatureSize()) return false;
        const uint64_t off[2] = {0, msg.size()};
        const uint8_t pad = 0;
        uint8_t ok = 0;
        VerifyBatch(pk.packed.data(), sig.data(), msg.empty() ? &pad : msg.data(), off, 1, &ok);
        return ok != 0;
    }

    // batches: seeds[n][32] -> pk[n][PublicKeySize], sk[n][PrivateKeySize]; messages as a blob + n + 1 offsets
    void DeriveKeyBatch(const uint8_t *seeds, size_t n, Bytes &pk, Bytes &sk) const {
        pk.assign(n * PublicKeySize(), 0);
        sk.assign(n * PrivateKeySize(), 0);
        if (!n) return;
        check(ed_dil_ ? circl_hip_eddilithium2_keygen(seeds, pk.data(), sk.data(), n, device)
                      : circl_hip_ed25519_keygen(seeds, pk.data(), sk.data(), n, device));
    }
    void SignBatch(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, size_t n, uint8_t *sig) const {
        check(ed_dil_ ? circl_hip_eddilithium2_sign(sk, msg_blob, msg_off, sig, n, device) : circl_hip_ed25519_sign(sk, msg_blob, msg_off, sig, n, device));
    }
    void VerifyBatch(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, size_t n, uint8_t *ok) const {
        check(ed_dil_ ? circl_hip_eddilithium2_verify(pk, sig, msg_blob, msg_off, ok, n, device)
                      : circl_hip_ed25519_verify(pk, sig, msg_blob, msg_off, ok, n, device));
    }

  private:
    bool ed_dil_;
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw sign::ErrDevice(std::string("circl-hip: error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
};

// sign/schemes.ByName("Ed25519") / ("Ed25519-Dilithium2")
inline const Scheme &ByName(const std::string &name) {
    static const Scheme ed(false), eddil(true);
    if (name == "Ed25519") return ed;
    if (name == "Ed25519-Dilithium2") return eddil;
    throw std::invalid_argument("unknown scheme " + name);
}

}  // namespace ed25519
}  // namespace circl
