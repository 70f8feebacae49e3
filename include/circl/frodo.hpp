// circl/frodo.hpp -- FrodoKEM-640-SHAKE on top of the HIP batch engine, shaped like the reference's kem.Scheme
// (kem/frodo/frodo640shake/frodo.go:423-547):
//
//   Name()                                   "FrodoKEM-640-SHAKE"
//   PublicKeySize() ... EncapsulationSeedSize()   9616, 19888, 48 (seed), 16 (shared key), 9720, 16
//   DeriveKeyPair(seed)                      -> {pk, sk}; throws kem::ErrSeedSize (the reference panics with it)
//   EncapsulateDeterministically(pk, seed)   -> {ct, ss}; throws kem::ErrSeedSize
//   Decapsulate(sk, ct)                      -> ss; throws kem::ErrCiphertextSize; a ciphertext that does not re-encrypt gives
//                                               SHAKE128(ct || s), not an error
//   UnmarshalBinaryPublicKey / PrivateKey    throw kem::ErrPubKeySize / kem::ErrPrivKeySize; keys are taken as stored
// plus batch forms over contiguous rows.  Everything runs on the GPU behind circl_hip_frodo640shake_*.  Link with -lcirclhip.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {
namespace frodo {

using kem::Bytes;

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
    const Bytes &MarshalBinary() const { return packed; }
    bool Equal(const PrivateKey &o) const { return scheme == o.scheme && packed == o.packed; }
    PublicKey Public() const;  // the pk stored in the key
};

class Scheme {
public:
    std::string Name() const { return "FrodoKEM-640-SHAKE"; }
    int PublicKeySize() const { return CIRCL_HIP_FRODO640SHAKE_PK_BYTES; }
    int PrivateKeySize() const { return CIRCL_HIP_FRODO640SHAKE_SK_BYTES; }
    int SeedSize() const { return CIRCL_HIP_FRODO640SHAKE_KEYSEED_BYTES; }
    int SharedKeySize() const { return CIRCL_HIP_FRODO640SHAKE_SS_BYTES; }
    int CiphertextSize() const { return CIRCL_HIP_FRODO640SHAKE_CT_BYTES; }
    int EncapsulationSeedSize() const { return CIRCL_HIP_FRODO640SHAKE_ENCSEED_BYTES; }

    std::pair<PublicKey, PrivateKey> DeriveKeyPair(const Bytes &seed, int device = 0) const {
        if ((int)seed.size() != SeedSize()) throw kem::ErrSeedSize();
        PublicKey pk{this, Bytes(PublicKeySize())};
        PrivateKey sk{this, Bytes(PrivateKeySize())};
        check(circl_hip_frodo640shake_keygen(seed.data(), pk.packed.data(), sk.packed.data(), 1, device));
        return {pk, sk};
    }
    std::pair<Bytes, Bytes> EncapsulateDeterministically(const PublicKey &pk, const Bytes &seed, int device = 0) const {
        if ((int)seed.size() != EncapsulationSeedSize()) throw kem::ErrSeedSize();
        if (pk.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ct(CiphertextSize()), ss(SharedKeySize());
        check(circl_hip_frodo640shake_encaps(pk.packed.data(), seed.data(), ct.data(), ss.data(), 1, device));
        return {ct, ss};
    }
    Bytes Decapsulate(const PrivateKey &sk, const Bytes &ct, int device = 0) const {
        if ((int)ct.size() != CiphertextSize()) throw kem::ErrCiphertextSize();
        if (sk.scheme != this) throw kem::ErrTypeMismatch();
        Bytes ss(SharedKeySize());
        check(circl_hip_frodo640shake_decaps(sk.packed.data(), ct.data(), ss.data(), 1, device));
        return ss;
    }
    PublicKey UnmarshalBinaryPublicKey(const Bytes &buf) const {
        if ((int)buf.size() != PublicKeySize()) throw kem::ErrPubKeySize();
        return PublicKey{this, buf};
    }
    PrivateKey UnmarshalBinaryPrivateKey(const Bytes &buf) const {
        if ((int)buf.size() != PrivateKeySize()) throw kem::ErrPrivKeySize();
        return PrivateKey{this, buf};
    }

    // batch forms: n contiguous rows each; device = CIRCL_HIP_ALL_DEVICES shards the batch
    void DeriveKeyPairBatch(const uint8_t *seeds, uint8_t *pks, uint8_t *sks, size_t n, int device = 0) const {
        check(circl_hip_frodo640shake_keygen(seeds, pks, sks, n, device));
    }
    void EncapsulateBatch(const uint8_t *pks, const uint8_t *seeds, uint8_t *cts, uint8_t *sss, size_t n, int device = 0) const {
        check(circl_hip_frodo640shake_encaps(pks, seeds, cts, sss, n, device));
    }
    void DecapsulateBatch(const uint8_t *sks, const uint8_t *cts, uint8_t *sss, size_t n, int device = 0) const {
        check(circl_hip_frodo640shake_decaps(sks, cts, sss, n, device));
    }

private:
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
};

inline const Scheme &Frodo640Shake() {
    static const Scheme s;
    return s;
}
inline PublicKey PrivateKey::Public() const {
    return PublicKey{scheme, Bytes(packed.begin() + CIRCL_HIP_FRODO640SHAKE_SS_BYTES,
                                   packed.begin() + CIRCL_HIP_FRODO640SHAKE_SS_BYTES + CIRCL_HIP_FRODO640SHAKE_PK_BYTES)};
}

}  // namespace frodo
}  // namespace circl
