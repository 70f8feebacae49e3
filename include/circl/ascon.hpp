// circl/ascon.hpp -- C++ mirror of the reference's cipher/ascon (Ascon v1.2: Ascon128, Ascon128a, Ascon80pq) over batches, behind
// circl_hip_ascon_*.  Header-only over the C ABI (link libcirclhip.so).
//
//   ascon::Cipher c(key, ascon::Ascon128);          ascon.New(key, mode): throws ErrKeySize / ErrMode
//   c.Seal(nonces, pts, aads) -> cts                Cipher.Seal per item: ct_i = ciphertext || 16-byte tag
//   c.Open(nonces, cts, aads) -> pts                Cipher.Open per item; LastOpenOk()[i] = 0 and an empty result where the tag of item i
//                                                   does not verify (the reference returns ErrDecryption and clears the plaintext)
//   c.NonceSize() = 16, c.Overhead() = 16, ModeKeySize(mode) = 16 / 16 / 20 (Mode.KeySize; throws ErrMode)
// One Cipher holds one key, as the reference's does; a batch under n keys is circl_hip_ascon_seal with a key stride.  Seal and Open
// always return fresh buffers: the reference's reuse of the input's storage is not offered.  The key is zeroed when the object goes away.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {
namespace ascon {

using kem::Bytes;
using List = std::vector<Bytes>;  // n byte strings; an empty list where n are expected means: every item is empty

enum Mode : int { Ascon128 = CIRCL_HIP_ASCON128, Ascon128a = CIRCL_HIP_ASCON128A, Ascon80pq = CIRCL_HIP_ASCON80PQ };
constexpr int KeySize = 16, KeySize80pq = 20, NonceSize = 16, TagSize = 16;

// ascon.go:312-317
struct ErrKeySize : kem::Error {
    ErrKeySize() : kem::Error("ascon: bad key size") {}
};
struct ErrNonceSize : kem::Error {
    ErrNonceSize() : kem::Error("ascon: bad nonce size") {}
};
struct ErrDecryption : kem::Error {
    ErrDecryption() : kem::Error("ascon: invalid ciphertext") {}
};
struct ErrMode : kem::Error {
    ErrMode() : kem::Error("ascon: invalid cipher mode") {}
};
struct ErrBatchSize : kem::Error {
    ErrBatchSize() : kem::Error("ascon: a list of another length than the batch") {}
};

inline int ModeKeySize(Mode m) {
    const size_t ks = circl_hip_ascon_key_size(m);
    if (!ks) throw ErrMode();
    return (int)ks;
}

class Cipher {
public:
    Cipher(const Bytes &key, Mode m, int device = 0) : key_(key), mode_(m), device_(device) {
        if ((int)key.size() != ModeKeySize(m)) throw ErrKeySize();
    }
    ~Cipher() {
        volatile uint8_t *p = key_.data();
        for (size_t i = 0; i < key_.size(); i++) p[i] = 0;
    }
    Cipher(const Cipher &) = default;
    Mode GetMode() const { return mode_; }
    int NonceSize() const { return ascon::NonceSize; }
    int Overhead() const { return TagSize; }

    // one ciphertext per nonce; pts and aads hold one item per nonce, or are empty (every item empty)
    List Seal(const List &nonces, const List &pts, const List &aads = {}) const {
        const size_t n = nonces.size();
        const Bytes nn = nonce_rows(nonces);
        const Ragged p(pts, n), a(aads, n);
        Bytes ct(p.bytes.size() + TagSize * n);
        check(circl_hip_ascon_seal(mode_, key_.data(), 0, nn.data(), p.blob(), p.offs(), a.blob(), a.offs(), ct.data(), n, device_));
        List r(n);
        for (size_t i = 0; i < n; i++) r[i].assign(ct.begin() + p.off[i] + TagSize * i, ct.begin() + p.off[i + 1] + TagSize * (i + 1));
        return r;
    }
    // one plaintext per nonce; an item whose tag does not verify gives an empty result and LastOpenOk()[i] = 0
    List Open(const List &nonces, const List &cts, const List &aads = {}) {
        const size_t n = nonces.size();
        if (cts.size() != n) throw ErrBatchSize();
        const Bytes nn = nonce_rows(nonces);
        List body(n);
        for (size_t i = 0; i < n; i++) {
            if (cts[i].size() < (size_t)TagSize) throw ErrDecryption();
            body[i].resize(cts[i].size() - TagSize);
        }
        const Ragged c(cts, n), p(body, n), a(aads, n);
        Bytes pt(p.bytes.size() + 1);
        last_ok_.assign(n, 0);
        check(circl_hip_ascon_open(mode_, key_.data(), 0, nn.data(), c.bytes.data(), p.off.data(), a.blob(), a.offs(), pt.data(), last_ok_.data(), n, device_));
        List r(n);
        for (size_t i = 0; i < n; i++)
            if (last_ok_[i]) r[i].assign(pt.begin() + p.off[i], pt.begin() + p.off[i + 1]);
        volatile uint8_t *w = pt.data();
        for (size_t i = 0; i < pt.size(); i++) w[i] = 0;
        return r;
    }
    const Bytes &LastOpenOk() const { return last_ok_; }

private:
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
    static Bytes nonce_rows(const List &nonces) {
        Bytes r;
        for (auto &x : nonces) {
            if (x.size() != (size_t)ascon::NonceSize) throw ErrNonceSize();
            r.insert(r.end(), x.begin(), x.end());
        }
        return r;
    }
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
    Bytes key_;
    Mode mode_;
    int device_;
    Bytes last_ok_;
};

}  // namespace ascon
}  // namespace circl
