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
// Below the KEM: the HPKE contexts (Suite, Sender, Receiver, Sealer, Opener) over batches, behind circl_hip_hpke_*.
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

// ---- HPKE contexts (hpke/hpke.go:74-270, hpke/aead.go) over batches --------------------------------------------------------------
//   Suite(kem, kdf, aead)                            kem 0x20 / 0x21, kdf 1 / 3 (HKDF-SHA256 / -SHA512), aead 3 (ChaCha20Poly1305) / 0xFFFF
//   suite.NewSender(pkR, info) / NewReceiver(skR, info)   n recipients and their n info strings (info may be {} = all empty)
//   sender.Setup(seeds) / SetupAuth / SetupPSK / SetupAuthPSK      -> {enc rows, Sealer}; deterministic: the caller draws the seeds
//   receiver.Setup(enc) / SetupAuth / SetupPSK / SetupAuthPSK      -> Opener
//   sealer.Seal(pts, aads) -> cts     opener.Open(cts, aads) -> pts     both: Export(exporter_contexts, length) -> n values
// A Sealer / Opener owns its n context rows and their sequence numbers (64-bit here; the reference's are 96-bit) and advances them as
// aead.go:54-76 does: after every Seal, and after an Open only for the items that verified.  Ok()[i] = 0 marks an item that is out of
// use (its setup failed: a low-order point, a psk that verifyPSKInputs refuses); Seal / Open / Export give it an empty result.
// Open additionally returns its own verdicts in LastOpenOk().  The context rows are zeroed when the object goes away.
struct ErrAEADSeqOverflows : kem::Error {
    ErrAEADSeqOverflows() : kem::Error("hpke: sequence number overflows") {}
};
struct ErrInvalidHPKESuite : kem::Error {
    ErrInvalidHPKESuite() : kem::Error("hpke: invalid HPKE suite") {}
};
struct ErrBatchSize : kem::Error {
    ErrBatchSize() : kem::Error("hpke: the batch's arrays differ in their number of items") {}
};

enum Mode : int { modeBase = 0, modePSK = 1, modeAuth = 2, modeAuthPSK = 3 };
using List = std::vector<Bytes>;  // n byte strings; an empty list where n are expected means: every item is empty

namespace detail {
inline void check(int rc) {
    if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
}
// a List as blob + offsets; blob() == nullptr when there are no bytes at all (the ABI's "every item is empty")
struct Ragged {
    Bytes bytes;
    std::vector<uint64_t> off;
    Ragged(const List &l, size_t n) : off(n + 1, 0) {
        if (!l.empty() && l.size() != n) throw ErrBatchSize();
        for (size_t i = 0; i < l.size(); i++) {
            bytes.insert(bytes.end(), l[i].begin(), l[i].end());
            off[i + 1] = bytes.size();
        }
    }
    const uint8_t *blob() const { return bytes.empty() ? nullptr : bytes.data(); }
    const uint64_t *offs() const { return bytes.empty() ? nullptr : off.data(); }
};
inline Bytes rows(const List &l, size_t n, size_t width) {  // n keys of `width` bytes as contiguous rows
    if (l.size() != n) throw ErrBatchSize();
    Bytes r;
    for (auto &k : l) {
        if (k.size() != width) throw kem::ErrPubKeySize();
        r.insert(r.end(), k.begin(), k.end());
    }
    return r;
}
inline void wipe(Bytes &b) {
    volatile uint8_t *p = b.data();
    for (size_t i = 0; i < b.size(); i++) p[i] = 0;
}
}  // namespace detail

class Suite {
public:
    Suite(int kem, int kdf, int aead) : kem_(kem), kdf_(kdf), aead_(aead) {}
    bool IsValid() const {
        return circl_hip_hpke_dhkem_key_size(kem_) && circl_hip_hpke_context_size(kdf_) &&
               (aead_ == CIRCL_HIP_HPKE_AEAD_CHACHA20POLY1305 || aead_ == CIRCL_HIP_HPKE_AEAD_EXPORT_ONLY);
    }
    int KEM() const { return kem_; }
    int KDF() const { return kdf_; }
    int AEAD() const { return aead_; }
    size_t KeySize() const { return circl_hip_hpke_dhkem_key_size(kem_); }
    size_t ContextSize() const { return circl_hip_hpke_context_size(kdf_); }
    bool operator==(const Suite &o) const { return kem_ == o.kem_ && kdf_ == o.kdf_ && aead_ == o.aead_; }

private:
    int kem_, kdf_, aead_;
};

// what a Sealer and an Opener share: the context rows, their sequence numbers, Export
class Context {
public:
    ~Context() { detail::wipe(ctx_); }
    Context(Context &&) = default;
    Context(const Context &) = delete;
    const Suite &GetSuite() const { return suite_; }
    size_t Size() const { return seq_.size(); }
    const Bytes &Ok() const { return ok_; }
    uint64_t Seq(size_t i) const { return seq_[i]; }
    List Export(const List &exporter_contexts, size_t length) const {
        const size_t n = Size();
        detail::Ragged e(exporter_contexts, n);
        Bytes out(n * length);
        detail::check(circl_hip_hpke_export(suite_.KDF(), suite_.KEM(), suite_.AEAD(), ctx_.data(), suite_.ContextSize(), e.blob(), e.offs(), length, out.data(), n,
                                            device_));
        List r(n);
        for (size_t i = 0; i < n; i++)
            if (ok_[i]) r[i].assign(out.begin() + i * length, out.begin() + (i + 1) * length);
        detail::wipe(out);
        return r;
    }

protected:
    Context(const Suite &s, Bytes ctx, Bytes ok, int device) : suite_(s), ctx_(std::move(ctx)), ok_(std::move(ok)), seq_(ok_.size(), 0), device_(device) {}
    void must_not_overflow() const {
        for (uint64_t q : seq_)
            if (q == UINT64_MAX) throw ErrAEADSeqOverflows();
    }
    Suite suite_;
    Bytes ctx_, ok_;
    std::vector<uint64_t> seq_;
    int device_;
};

class Sealer : public Context {
public:
    Sealer(const Suite &s, Bytes ctx, Bytes ok, int device) : Context(s, std::move(ctx), std::move(ok), device) {}
    // aead.go:54-63: ct_i = Seal(key_i, base_nonce_i XOR seq_i, pt_i, aad_i); every sequence number advances
    List Seal(const List &pts, const List &aads = {}) {
        const size_t n = Size();
        must_not_overflow();
        detail::Ragged p(pts, n), a(aads, n);
        Bytes ct(p.bytes.size() + 16 * n);
        detail::check(circl_hip_hpke_seal(suite_.AEAD(), ctx_.data(), suite_.ContextSize(), seq_.data(), p.blob(), p.off.data(), a.blob(), a.offs(), ct.data(), n,
                                          device_));
        List r(n);
        for (size_t i = 0; i < n; i++) {
            if (ok_[i]) r[i].assign(ct.begin() + p.off[i] + 16 * i, ct.begin() + p.off[i + 1] + 16 * (i + 1));
            seq_[i]++;
        }
        return r;
    }
};

class Opener : public Context {
public:
    Opener(const Suite &s, Bytes ctx, Bytes ok, int device) : Context(s, std::move(ctx), std::move(ok), device) {}
    // aead.go:65-76: pt_i = Open(...); the sequence number of an item advances only if its tag verified
    List Open(const List &cts, const List &aads = {}) {
        const size_t n = Size();
        must_not_overflow();
        if (cts.size() != n) throw ErrBatchSize();
        List body(n);
        for (size_t i = 0; i < n; i++) {
            if (cts[i].size() < 16) throw kem::ErrCiphertextSize();
            body[i].resize(cts[i].size() - 16);
        }
        detail::Ragged c(cts, n), p(body, n), a(aads, n);
        Bytes pt(p.bytes.size() + 1);
        last_ok_.assign(n, 0);
        detail::check(circl_hip_hpke_open(suite_.AEAD(), ctx_.data(), suite_.ContextSize(), seq_.data(), c.bytes.data(), p.off.data(), a.blob(), a.offs(), pt.data(),
                                          last_ok_.data(), n, device_));
        List r(n);
        for (size_t i = 0; i < n; i++) {
            last_ok_[i] = last_ok_[i] && ok_[i];
            if (!last_ok_[i]) continue;
            r[i].assign(pt.begin() + p.off[i], pt.begin() + p.off[i + 1]);
            seq_[i]++;
        }
        detail::wipe(pt);
        return r;
    }
    const Bytes &LastOpenOk() const { return last_ok_; }

private:
    Bytes last_ok_;
};

class Sender {
public:
    // hpke.go NewSender: n recipients' public keys and their info strings
    Sender(const Suite &s, const std::vector<PublicKey> &pkR, List info, int device = 0) : suite_(s), n_(pkR.size()), info_(std::move(info)), device_(device) {
        if (!s.IsValid()) throw ErrInvalidHPKESuite();
        for (auto &k : pkR) {
            if (k.packed.size() != s.KeySize()) throw kem::ErrPubKeySize();
            pkR_.insert(pkR_.end(), k.packed.begin(), k.packed.end());
        }
    }
    std::pair<List, Sealer> Setup(const List &seeds) const { return setup(modeBase, seeds, nullptr, {}, {}); }
    std::pair<List, Sealer> SetupAuth(const List &seeds, const std::vector<PrivateKey> &skS) const { return setup(modeAuth, seeds, &skS, {}, {}); }
    std::pair<List, Sealer> SetupPSK(const List &seeds, const List &psk, const List &pskID) const { return setup(modePSK, seeds, nullptr, psk, pskID); }
    std::pair<List, Sealer> SetupAuthPSK(const List &seeds, const std::vector<PrivateKey> &skS, const List &psk, const List &pskID) const {
        return setup(modeAuthPSK, seeds, &skS, psk, pskID);
    }

private:
    std::pair<List, Sealer> setup(int mode, const List &seeds, const std::vector<PrivateKey> *skS, const List &psk, const List &pskID) const {
        const size_t N = suite_.KeySize(), CS = suite_.ContextSize();
        Bytes ikm = detail::rows(seeds, n_, N), sk, pk;
        if (skS) {
            if (skS->size() != n_) throw ErrBatchSize();
            for (auto &k : *skS) {
                if (k.packed.size() != N || k.pub.size() != N) throw kem::ErrPrivKeySize();
                sk.insert(sk.end(), k.packed.begin(), k.packed.end());
                pk.insert(pk.end(), k.pub.begin(), k.pub.end());
            }
        }
        detail::Ragged info(info_, n_), p(psk, n_), id(pskID, n_);
        const bool with_psk = mode & 1;
        Bytes enc(n_ * N), ctx(n_ * CS), ok(n_);
        detail::check(circl_hip_hpke_setup_sender(suite_.KEM(), suite_.KDF(), suite_.AEAD(), mode, pkR_.data(), ikm.data(), skS ? sk.data() : nullptr,
                                                  skS ? pk.data() : nullptr, info.blob(), info.offs(), with_psk ? p.blob() : nullptr, with_psk ? p.offs() : nullptr,
                                                  with_psk ? id.blob() : nullptr, with_psk ? id.offs() : nullptr, enc.data(), ctx.data(), ok.data(), n_, device_));
        detail::wipe(ikm);
        detail::wipe(sk);
        List encs(n_);
        for (size_t i = 0; i < n_; i++)
            if (ok[i]) encs[i].assign(enc.begin() + i * N, enc.begin() + (i + 1) * N);
        return {std::move(encs), Sealer(suite_, std::move(ctx), std::move(ok), device_)};
    }
    Suite suite_;
    size_t n_;
    Bytes pkR_;
    List info_;
    int device_;
};

class Receiver {
public:
    // hpke.go NewReceiver: n recipients' private keys (each carries its public key) and their info strings
    Receiver(const Suite &s, const std::vector<PrivateKey> &skR, List info, int device = 0) : suite_(s), n_(skR.size()), info_(std::move(info)), device_(device) {
        if (!s.IsValid()) throw ErrInvalidHPKESuite();
        for (auto &k : skR) {
            if (k.packed.size() != s.KeySize() || k.pub.size() != s.KeySize()) throw kem::ErrPrivKeySize();
            skR_.insert(skR_.end(), k.packed.begin(), k.packed.end());
            pkR_.insert(pkR_.end(), k.pub.begin(), k.pub.end());
        }
    }
    ~Receiver() { detail::wipe(skR_); }
    Opener Setup(const List &enc) const { return setup(modeBase, enc, nullptr, {}, {}); }
    Opener SetupAuth(const List &enc, const std::vector<PublicKey> &pkS) const { return setup(modeAuth, enc, &pkS, {}, {}); }
    Opener SetupPSK(const List &enc, const List &psk, const List &pskID) const { return setup(modePSK, enc, nullptr, psk, pskID); }
    Opener SetupAuthPSK(const List &enc, const std::vector<PublicKey> &pkS, const List &psk, const List &pskID) const {
        return setup(modeAuthPSK, enc, &pkS, psk, pskID);
    }

private:
    Opener setup(int mode, const List &enc, const std::vector<PublicKey> *pkS, const List &psk, const List &pskID) const {
        const size_t N = suite_.KeySize(), CS = suite_.ContextSize();
        if (enc.size() != n_) throw ErrBatchSize();
        Bytes e, pk;
        for (auto &c : enc) {
            if (c.size() != N) throw kem::ErrCiphertextSize();
            e.insert(e.end(), c.begin(), c.end());
        }
        if (pkS) {
            if (pkS->size() != n_) throw ErrBatchSize();
            for (auto &k : *pkS) {
                if (k.packed.size() != N) throw kem::ErrPubKeySize();
                pk.insert(pk.end(), k.packed.begin(), k.packed.end());
            }
        }
        detail::Ragged info(info_, n_), p(psk, n_), id(pskID, n_);
        const bool with_psk = mode & 1;
        Bytes ctx(n_ * CS), ok(n_);
        detail::check(circl_hip_hpke_setup_receiver(suite_.KEM(), suite_.KDF(), suite_.AEAD(), mode, skR_.data(), pkR_.data(), e.data(), pkS ? pk.data() : nullptr,
                                                    info.blob(), info.offs(), with_psk ? p.blob() : nullptr, with_psk ? p.offs() : nullptr,
                                                    with_psk ? id.blob() : nullptr, with_psk ? id.offs() : nullptr, ctx.data(), ok.data(), n_, device_));
        return Opener(suite_, std::move(ctx), std::move(ok), device_);
    }
    Suite suite_;
    size_t n_;
    Bytes skR_, pkR_;
    List info_;
    int device_;
};

}  // namespace hpke
}  // namespace circl
