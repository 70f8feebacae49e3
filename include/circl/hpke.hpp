// circl/hpke.hpp -- the HPKE DHKEMs over X25519 and X448 on top of the HIP batch engine, shaped like the reference's kem.AuthScheme
// for hpke.KEM_X25519_HKDF_SHA256 (0x20) and hpke.KEM_X448_HKDF_SHA512 (0x21) (hpke/algs.go:266-277, hpke/kembase.go, hpke/xkem.go):
//
//   Name()                                         "HPKE_KEM_X25519_HKDF_SHA256" / "HPKE_KEM_X448_HKDF_SHA512"
//   PublicKeySize() ... EncapsulationSeedSize()        32 / 56 for keys, seeds and ciphertexts; SharedKeySize() 32 / 64
//   DeriveKeyPair(seed)                            -> {pk, sk}; throws kem::ErrSeedSize (the reference panics with it)
//   EncapsulateDeterministically(pk, seed)         -> {ct, ss}
//   Decapsulate(sk, ct)                            -> ss
//   AuthEncapsulateDeterministically(pkR, skS, seed) -> {ct, ss}
//   AuthDecapsulate(skR, ct, pkS)                  -> ss
//   UnmarshalBinaryPublicKey / PrivateKey          throw kem::ErrPubKeySize / kem::ErrPrivKeySize; keys are taken as stored
// A low-order point (x25519.Shared / x448.Shared return false) throws hpke::ErrInvalidKEMSharedSecret.  A private key carries its
// public key (the reference caches Public()), so Decapsulate and the auth forms do not recompute it.  Plus batch forms over
// contiguous rows, with an ok array instead of exceptions.  The random forms (GenerateKeyPair, Encapsulate) stay with the caller:
// draw the seed and call the deterministic form.  Everything runs on the GPU behind circl_hip_hpke_dhkem_*.  Link with -lcirclhip.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {
namespace hpke {

using kem::Bytes;

struct ErrInvalidKEMSharedSecret : kem::Error {
    ErrInvalidKEMSharedSecret() : kem::Error("hpke: invalid KEM shared secret") {}
};

class Scheme;
struct PublicKey {
    const Scheme *scheme;
    Bytes packed;
    const Bytes &MarshalBinary() const { return packed; }
    bool Equal(const PublicKey &o) const { return scheme == o.scheme && packed == o.packed; }
};
struct PrivateKey {
    const Scheme *scheme;
    Bytes packed;
    Bytes pub;  // KeyGen(packed), filled by DeriveKeyPair / UnmarshalBinaryPrivateKey
    const Bytes &MarshalBinary() const { return packed; }
    bool Equal(const PrivateKey &o) const { return scheme == o.scheme && packed == o.packed; }
    PublicKey Public() const { return PublicKey{scheme, pub}; }
};

class Scheme {
public:
    explicit Scheme(int kem_id) : id_(kem_id), n_((int)circl_hip_hpke_dhkem_key_size(kem_id)), s_((int)circl_hip_hpke_dhkem_ss_size(kem_id)) {
        if (!n_) throw kem::ErrDevice("unknown HPKE KEM id");
    }
    int ID() const { return id_; }
    std::string Name() const { return id_ == CIRCL_HIP_HPKE_KEM_X25519_HKDF_SHA256 ? "HPKE_KEM_X25519_HKDF_SHA256" : "HPKE_KEM_X448_HKDF_SHA512"; }
    int PublicKeySize() const { return n_; }
    int PrivateKeySize() const { return n_; }
    int SeedSize() const { return n_; }
    int CiphertextSize() const { return n_; }
    int EncapsulationSeedSize() const { return n_; }
    int SharedKeySize() const { return s_; }

    std::pair<PublicKey, PrivateKey> DeriveKeyPair(const Bytes &seed, int device = 0) const {
        if ((int)seed.size() != SeedSize()) throw kem::ErrSeedSize();
        PrivateKey sk{this, Bytes(n_), Bytes(n_)};
        check(circl_hip_hpke_dhkem_derive_keypair(id_, seed.data(), sk.packed.data(), sk.pub.data(), 1, device));
        return {sk.Public(), sk};
    }
    std::pair<Bytes, Bytes> EncapsulateDeterministically(const PublicKey &pk, const Bytes &seed, int device = 0) const {
        if ((int)seed.size() != EncapsulationSeedSize()) throw kem::ErrSeedSize();
        if (pk.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ct(n_), ss(s_);
        uint8_t ok = 0;
        check(circl_hip_hpke_dhkem_encap(id_, pk.packed.data(), seed.data(), ct.data(), ss.data(), &ok, 1, device));
        if (!ok) throw ErrInvalidKEMSharedSecret();
        return {ct, ss};
    }
    Bytes Decapsulate(const PrivateKey &sk, const Bytes &ct, int device = 0) const {
        if ((int)ct.size() != CiphertextSize()) throw kem::ErrCiphertextSize();
        if (sk.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ss(s_);
        uint8_t ok = 0;
        check(circl_hip_hpke_dhkem_decap(id_, sk.packed.data(), sk.pub.data(), ct.data(), ss.data(), &ok, 1, device));
        if (!ok) throw ErrInvalidKEMSharedSecret();
        return ss;
    }
    std::pair<Bytes, Bytes> AuthEncapsulateDeterministically(const PublicKey &pkR, const PrivateKey &skS, const Bytes &seed, int device = 0) const {
        if ((int)seed.size() != EncapsulationSeedSize()) throw kem::ErrSeedSize();
        if (pkR.scheme != this || skS.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ct(n_), ss(s_);
        uint8_t ok = 0;
        check(circl_hip_hpke_dhkem_auth_encap(id_, pkR.packed.data(), skS.packed.data(), skS.pub.data(), seed.data(), ct.data(), ss.data(), &ok, 1, device));
        if (!ok) throw ErrInvalidKEMSharedSecret();
        return {ct, ss};
    }
    Bytes AuthDecapsulate(const PrivateKey &skR, const Bytes &ct, const PublicKey &pkS, int device = 0) const {
        if ((int)ct.size() != CiphertextSize()) throw kem::ErrCiphertextSize();
        if (skR.scheme != this || pkS.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ss(s_);
        uint8_t ok = 0;
        check(circl_hip_hpke_dhkem_auth_decap(id_, skR.packed.data(), skR.pub.data(), ct.data(), pkS.packed.data(), ss.data(), &ok, 1, device));
        if (!ok) throw ErrInvalidKEMSharedSecret();
        return ss;
    }
    PublicKey UnmarshalBinaryPublicKey(const Bytes &buf) const {
        if ((int)buf.size() != PublicKeySize()) throw kem::ErrPubKeySize();
        return PublicKey{this, buf};
    }
    PrivateKey UnmarshalBinaryPrivateKey(const Bytes &buf, int device = 0) const {  // pub = KeyGen(buf): the bare scalar multiplication
        if ((int)buf.size() != PrivateKeySize()) throw kem::ErrPrivKeySize();
        PrivateKey sk{this, buf, Bytes(n_)};
        check(id_ == CIRCL_HIP_HPKE_KEM_X25519_HKDF_SHA256 ? circl_hip_x25519(buf.data(), nullptr, sk.pub.data(), nullptr, 1, device)
                                                          : circl_hip_x448(buf.data(), nullptr, sk.pub.data(), nullptr, 1, device));
        return sk;
    }

    // batch forms: n contiguous rows each; ok[i] = 0 (and zero rows) where the reference returns ErrInvalidKEMSharedSecret; own public
    // keys (pkR of the decapsulations, pkS of AuthEncapsulate) may be nullptr; device = CIRCL_HIP_ALL_DEVICES shards the batch
    void DeriveKeyPairBatch(const uint8_t *seeds, uint8_t *sks, uint8_t *pks, size_t n, int device = 0) const {
        check(circl_hip_hpke_dhkem_derive_keypair(id_, seeds, sks, pks, n, device));
    }
    void EncapsulateBatch(const uint8_t *pkR, const uint8_t *seeds, uint8_t *cts, uint8_t *sss, uint8_t *ok, size_t n, int device = 0) const {
        check(circl_hip_hpke_dhkem_encap(id_, pkR, seeds, cts, sss, ok, n, device));
    }
    void DecapsulateBatch(const uint8_t *skR, const uint8_t *pkR, const uint8_t *cts, uint8_t *sss, uint8_t *ok, size_t n, int device = 0) const {
        check(circl_hip_hpke_dhkem_decap(id_, skR, pkR, cts, sss, ok, n, device));
    }
    void AuthEncapsulateBatch(const uint8_t *pkR, const uint8_t *skS, const uint8_t *pkS, const uint8_t *seeds, uint8_t *cts, uint8_t *sss, uint8_t *ok,
                              size_t n, int device = 0) const {
        check(circl_hip_hpke_dhkem_auth_encap(id_, pkR, skS, pkS, seeds, cts, sss, ok, n, device));
    }
    void AuthDecapsulateBatch(const uint8_t *skR, const uint8_t *pkR, const uint8_t *cts, const uint8_t *pkS, uint8_t *sss, uint8_t *ok, size_t n,
                              int device = 0) const {
        check(circl_hip_hpke_dhkem_auth_decap(id_, skR, pkR, cts, pkS, sss, ok, n, device));
    }

private:
    int id_, n_, s_;
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
};

inline const Scheme &KEM_X25519_HKDF_SHA256() {
    static const Scheme s(CIRCL_HIP_HPKE_KEM_X25519_HKDF_SHA256);
    return s;
}
inline const Scheme &KEM_X448_HKDF_SHA512() {
    static const Scheme s(CIRCL_HIP_HPKE_KEM_X448_HKDF_SHA512);
    return s;
}

}  // namespace hpke
}  // namespace circl
