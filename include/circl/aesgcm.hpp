// circl/aesgcm.hpp -- C++ mirror of Go's cipher.AEAD for AES-128-GCM and AES-256-GCM (what hpke/aead.go makes of AEAD ids 1 and 2:
// aes.NewCipher + cipher.NewGCM) over batches, behind circl_hip_aesgcm_*.  Header-only over the C ABI (link libcirclhip.so).
//
//   aesgcm::Cipher c(key);                          aes.NewCipher(key) + cipher.NewGCM: 16 or 32 bytes, else ErrKeySize
//   c.Seal(nonces, pts, aads) -> cts                AEAD.Seal per item: ct_i = ciphertext || 16-byte tag
//   c.Open(nonces, cts, aads) -> pts                AEAD.Open per item; LastOpenOk()[i] = 0 and an empty result where the tag of item i
//                                                   does not verify ("cipher: message authentication failed")
//   c.SealSeq(base_nonce, first_seq, pts, aads)     one HPKE context sealing a run of records: item i under base_nonce XOR BE96(first_seq + i)
//   c.OpenSeq(base_nonce, first_seq, cts, aads)     (hpke/aead.go:47-52)
//   c.NonceSize() = 12, c.Overhead() = 16
// One Cipher holds one key, as Go's does; a batch under n keys is circl_hip_aesgcm_seal with a key stride.  Distinct nonces under
// that key are the caller's duty, as with cipher.AEAD.  Seal and Open always return fresh buffers: Go's reuse of dst is not offered.
// The key is zeroed when the object goes away.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {
namespace aesgcm {

using kem::Bytes;
using List = std::vector<Bytes>;  // n byte strings; an empty list where n are expected means: every item is empty

constexpr int KeySize128 = CIRCL_HIP_AES128GCM, KeySize256 = CIRCL_HIP_AES256GCM, NonceSize = 12, TagSize = 16;

struct ErrKeySize : kem::Error {
    ErrKeySize() : kem::Error("crypto/aes: invalid key size") {}
};
struct ErrNonceSize : kem::Error {
    ErrNonceSize() : kem::Error("crypto/cipher: incorrect nonce length given to GCM") {}
};
struct ErrOpen : kem::Error {
    ErrOpen() : kem::Error("cipher: message authentication failed") {}
};
struct ErrBatchSize : kem::Error {
    ErrBatchSize() : kem::Error("aesgcm: a list of another length than the batch") {}
};

class Cipher {
public:
    explicit Cipher(const Bytes &key, int device = 0) : key_(key), device_(device) {
        if (key.size() != (size_t)KeySize128 && key.size() != (size_t)KeySize256) throw ErrKeySize();
    }
    ~Cipher() {
        volatile uint8_t *p = key_.data();
        for (size_t i = 0; i < key_.size(); i++) p[i] = 0;
    }
    Cipher(const Cipher &) = default;
    int NonceSize() const { return aesgcm::NonceSize; }
    int Overhead() const { return TagSize; }

    // one ciphertext per nonce; pts and aads hold one item per nonce, or are empty (every item empty)
    List Seal(const List &nonces, const List &pts, const List &aads = {}) const {
        const Bytes nn = nonce_rows(nonces);
        return seal(nn, aesgcm::NonceSize, {}, nonces.size(), pts, aads);
    }
    // one plaintext per nonce; an item whose tag does not verify gives an empty result and LastOpenOk()[i] = 0
    List Open(const List &nonces, const List &cts, const List &aads = {}) {
        if (cts.size() != nonces.size()) throw ErrBatchSize();
        const Bytes nn = nonce_rows(nonces);
        return open(nn, aesgcm::NonceSize, {}, cts, aads);
    }
    // item i under the nonce base_nonce XOR BE96(first_seq + i)
    List SealSeq(const Bytes &base_nonce, uint64_t first_seq, const List &pts, const List &aads = {}) const {
        if (base_nonce.size() != (size_t)aesgcm::NonceSize) throw ErrNonceSize();
        return seal(base_nonce, 0, seqs(first_seq, pts.size()), pts.size(), pts, aads);
    }
    List OpenSeq(const Bytes &base_nonce, uint64_t first_seq, const List &cts, const List &aads = {}) {
        if (base_nonce.size() != (size_t)aesgcm::NonceSize) throw ErrNonceSize();
        return open(base_nonce, 0, seqs(first_seq, cts.size()), cts, aads);
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
    List seal(const Bytes &nn, size_t nonce_stride, const std::vector<uint64_t> &seq, size_t n, const List &pts, const List &aads) const {
        const Ragged p(pts, n), a(aads, n);
        Bytes ct(p.bytes.size() + TagSize * n);
        check(circl_hip_aesgcm_seal((int)key_.size(), key_.data(), 0, nn.data(), nonce_stride, seq.empty() ? nullptr : seq.data(), p.blob(), p.offs(), a.blob(),
                                    a.offs(), ct.data(), n, device_));
        List r(n);
        for (size_t i = 0; i < n; i++) r[i].assign(ct.begin() + p.off[i] + TagSize * i, ct.begin() + p.off[i + 1] + TagSize * (i + 1));
        return r;
    }
    List open(const Bytes &nn, size_t nonce_stride, const std::vector<uint64_t> &seq, const List &cts, const List &aads) {
        const size_t n = cts.size();
        List body(n);
        for (size_t i = 0; i < n; i++) {
            if (cts[i].size() < (size_t)TagSize) throw ErrOpen();
            body[i].resize(cts[i].size() - TagSize);
        }
        const Ragged c(cts, n), p(body, n), a(aads, n);
        Bytes pt(p.bytes.size() + 1);
        last_ok_.assign(n, 0);
        check(circl_hip_aesgcm_open((int)key_.size(), key_.data(), 0, nn.data(), nonce_stride, seq.empty() ? nullptr : seq.data(), c.bytes.data(), p.off.data(),
                                    a.blob(), a.offs(), pt.data(), last_ok_.data(), n, device_));
        List r(n);
        for (size_t i = 0; i < n; i++)
            if (last_ok_[i]) r[i].assign(pt.begin() + p.off[i], pt.begin() + p.off[i + 1]);
        volatile uint8_t *w = pt.data();
        for (size_t i = 0; i < pt.size(); i++) w[i] = 0;
        return r;
    }
    static std::vector<uint64_t> seqs(uint64_t first, size_t n) {
        std::vector<uint64_t> s(n ? n : 1);
        for (size_t i = 0; i < s.size(); i++) s[i] = first + i;
        return s;
    }
    static Bytes nonce_rows(const List &nonces) {
        Bytes r;
        for (auto &x : nonces) {
            if (x.size() != (size_t)aesgcm::NonceSize) throw ErrNonceSize();
            r.insert(r.end(), x.begin(), x.end());
        }
        return r;
    }
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
    Bytes key_;
    int device_;
    Bytes last_ok_;
};

}  // namespace aesgcm
}  // namespace circl
