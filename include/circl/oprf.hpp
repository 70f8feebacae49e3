// circl/oprf.hpp -- the ristretto255 group and OPRF, VOPRF and POPRF (suite ristretto255-SHA512) on top of the HIP batch engine,
// shaped like the reference's group.Ristretto255 (group/ristretto255.go) and oprf package (oprf/keys.go, client.go, server.go), over
// batches:
//
//   group::Ristretto255::HashToElement(msgs, dst) / HashToScalar(msgs, dst)     -> n encodings of 32 bytes
//   group::Ristretto255::Mul(scalars, elems) / MulGen(scalars) / MulInverse     -> {n encodings, ok}; one scalar serves the batch
//   oprf::DeriveKey(mode, seed, info)                                           -> PrivateKey (carries its public key)
//   oprf::Client(mode).DeterministicBlind(inputs, blinds)                       -> {FinalizeData, EvaluationRequest}
//   oprf::Server(key).Evaluate(request)                                         -> Evaluation           (base mode)
//   oprf::Client(mode).Finalize(finalizeData, evaluation)                       -> n outputs of 64 bytes (base mode)
//   oprf::Server(key).FullEvaluate(inputs) / oprf::VerifiableServer(key).FullEvaluate(inputs)   -> n outputs
//   oprf::VerifiableServer(key).Evaluate(request, r) / oprf::PartialObliviousServer(key).Evaluate(request, info, r)  -> Evaluation with its proof
//   oprf::VerifiableClient(pkS).Finalize(finalizeData, evaluation) / oprf::PartialObliviousClient(pkS).Finalize(.., info)  -> n outputs
//   oprf::PartialObliviousServer(key).FullEvaluate(inputs, info)                                        -> n outputs
// A verifiable call is ONE request (the reference's batch under one proof, 1 to 65535 elements); r is the proof's randomness.
// The library has no random number generator: the caller draws the blinds and r (the reference's Blind is DeterministicBlind on blinds it
// draws).  As in the reference, a call fails as a whole: an input the protocol refuses throws ErrInvalidInput, a zero or
// non-canonical scalar or key ErrInvalidScalar, an element that does not decode or is the identity ErrInvalidElement.  Decoding is
// strict RFC 9496 (include/circl_hip.h).  A proof that does not verify throws ErrInvalidProof and no output leaves the call.
// Everything runs on the GPU behind circl_hip_ristretto255_*, circl_hip_oprf_* and circl_hip_dleq_*.  Link with -lcirclhip.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {

namespace oprf {
using kem::Bytes;
using List = std::vector<Bytes>;  // n byte strings

struct ErrInvalidInput : kem::Error {
    ErrInvalidInput() : kem::Error("oprf: invalid input") {}
};
struct ErrInvalidScalar : kem::Error {
    ErrInvalidScalar() : kem::Error("oprf: a scalar is zero or not canonical") {}
};
struct ErrInvalidElement : kem::Error {
    ErrInvalidElement() : kem::Error("oprf: an element does not decode or is the identity") {}
};
struct ErrBatchSize : kem::Error {
    ErrBatchSize() : kem::Error("oprf: the batch's arrays differ in their number of items") {}
};
struct ErrInvalidProof : kem::Error {
    ErrInvalidProof() : kem::Error("oprf: the proof does not verify") {}
};
struct ErrModeNotServed : kem::Error {
    ErrModeNotServed() : kem::Error("oprf: this operation of the verifiable modes needs a proof and is not served") {}
};

namespace detail {
inline void check(int rc) {
    if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
}
// a List as blob + offsets (never a NULL blob: an empty batch of bytes still has its offsets)
struct Ragged {
    Bytes bytes;
    std::vector<uint64_t> off;
    explicit Ragged(const List &l) : off(l.size() + 1, 0) {
        for (size_t i = 0; i < l.size(); i++) {
            bytes.insert(bytes.end(), l[i].begin(), l[i].end());
            off[i + 1] = bytes.size();
        }
        bytes.push_back(0);
    }
    const uint8_t *blob() const { return bytes.data(); }
    const uint64_t *offs() const { return off.data(); }
};
// n rows of 32 bytes, contiguous; one row where `shared`
inline Bytes rows(const List &l, size_t n) {
    if (l.size() != n) throw ErrBatchSize();
    Bytes r;
    for (auto &k : l) {
        if (k.size() != 32) throw ErrBatchSize();
        r.insert(r.end(), k.begin(), k.end());
    }
    return r;
}
inline List unrows(const Bytes &b, size_t width) {
    List l(b.size() / width);
    for (size_t i = 0; i < l.size(); i++) l[i].assign(b.begin() + i * width, b.begin() + (i + 1) * width);
    return l;
}
inline void wipe(Bytes &b) {
    volatile uint8_t *p = b.data();
    for (size_t i = 0; i < b.size(); i++) p[i] = 0;
}
inline bool all_ok(const Bytes &ok) {
    for (uint8_t o : ok)
        if (!o) return false;
    return true;
}
inline bool scalar_usable(const Bytes &k) {  // below L and not zero (the cheap host-side reading of a 32-byte little-endian value)
    static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                  0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
    if (k.size() != 32) return false;
    bool zero = true;
    for (uint8_t b : k) zero = zero && b == 0;
    if (zero) return false;
    for (int i = 31; i >= 0; i--)
        if (k[i] != L[i]) return k[i] < L[i];
    return false;
}
}  // namespace detail
}  // namespace oprf

namespace group {
using oprf::Bytes;
using oprf::List;

// group.Ristretto255 over batches: elements and scalars are their 32-byte encodings
struct Ristretto255 {
    static List HashToElement(const List &msgs, const Bytes &dst, int device = 0) {
        const oprf::detail::Ragged m(msgs);
        Bytes out(32 * msgs.size());
        oprf::detail::check(circl_hip_ristretto255_hash_to_group(m.blob(), m.offs(), dst.data(), dst.size(), out.data(), msgs.size(), device));
        return oprf::detail::unrows(out, 32);
    }
    static List HashToScalar(const List &msgs, const Bytes &dst, int device = 0) {
        const oprf::detail::Ragged m(msgs);
        Bytes out(32 * msgs.size());
        oprf::detail::check(circl_hip_ristretto255_hash_to_scalar(m.blob(), m.offs(), dst.data(), dst.size(), out.data(), msgs.size(), device));
        return oprf::detail::unrows(out, 32);
    }
    // scalars: n of them, or one for the batch; elems empty: the generator (then n = scalars.size()).  -> {n encodings, ok}
    static std::pair<List, Bytes> Mul(const List &scalars, const List &elems, bool invert = false, int device = 0) {
        const size_t n = elems.empty() ? scalars.size() : elems.size();
        const bool shared = scalars.size() == 1 && n != 1;
        Bytes sc = oprf::detail::rows(scalars, shared ? 1 : n), el = elems.empty() ? Bytes() : oprf::detail::rows(elems, n), out(32 * n), ok(n);
        oprf::detail::check(circl_hip_ristretto255_scalar_mult(sc.data(), shared ? 0 : 32, elems.empty() ? nullptr : el.data(), invert ? CIRCL_HIP_R255_INVERT : 0,
                                                               out.data(), ok.data(), n, device));
        oprf::detail::wipe(sc);
        return {oprf::detail::unrows(out, 32), ok};
    }
    static std::pair<List, Bytes> MulGen(const List &scalars, int device = 0) { return Mul(scalars, {}, false, device); }
    static std::pair<List, Bytes> MulInverse(const List &scalars, const List &elems, int device = 0) { return Mul(scalars, elems, true, device); }
};
}  // namespace group

namespace oprf {

enum Mode : int { BaseMode = CIRCL_HIP_OPRF_MODE_OPRF, VerifiableMode = CIRCL_HIP_OPRF_MODE_VOPRF, PartialObliviousMode = CIRCL_HIP_OPRF_MODE_POPRF };

struct PublicKey {
    Bytes e;
    const Bytes &MarshalBinary() const { return e; }
};
struct PrivateKey {
    Bytes k, pub;
    const Bytes &MarshalBinary() const { return k; }
    PublicKey Public() const { return PublicKey{pub}; }
};

// oprf.DeriveKey(suite, mode, seed, info) for n (seed, info) pairs
inline std::vector<PrivateKey> DeriveKeys(Mode mode, const List &seeds, const List &infos, int device = 0) {
    const size_t n = seeds.size();
    if (infos.size() != n) throw ErrBatchSize();
    Bytes s = detail::rows(seeds, n), sk(32 * n), pk(32 * n), ok(n);
    const detail::Ragged info(infos);
    detail::check(circl_hip_oprf_derive_keypair(mode, s.data(), info.blob(), info.offs(), sk.data(), pk.data(), ok.data(), n, device));
    detail::wipe(s);
    if (!detail::all_ok(ok)) throw ErrInvalidInput();
    std::vector<PrivateKey> keys(n);
    for (size_t i = 0; i < n; i++) keys[i] = PrivateKey{Bytes(sk.begin() + 32 * i, sk.begin() + 32 * (i + 1)), Bytes(pk.begin() + 32 * i, pk.begin() + 32 * (i + 1))};
    detail::wipe(sk);
    return keys;
}
inline PrivateKey DeriveKey(Mode mode, const Bytes &seed, const Bytes &info, int device = 0) { return DeriveKeys(mode, {seed}, {info}, device)[0]; }

struct EvaluationRequest {
    List Elements;
};
struct Evaluation {
    List Elements;
    Bytes Proof;  // c || s, 64 bytes: the verifiable modes; empty in base mode
};
struct FinalizeData {
    List inputs, blinds;
    EvaluationRequest evalReq;
};

class Client {
public:
    explicit Client(Mode mode, int device = 0) : mode_(mode), device_(device) {}
    // client.go DeterministicBlind
    std::pair<FinalizeData, EvaluationRequest> DeterministicBlind(const List &inputs, const List &blinds) const {
        const size_t n = inputs.size();
        if (n == 0) throw ErrInvalidInput();
        Bytes b = detail::rows(blinds, n), out(32 * n), ok(n);
        const detail::Ragged in(inputs);
        detail::check(circl_hip_oprf_blind(mode_, in.blob(), in.offs(), b.data(), out.data(), ok.data(), n, device_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            for (auto &k : blinds)
                if (!detail::scalar_usable(k)) throw ErrInvalidScalar();
            throw ErrInvalidInput();
        }
        EvaluationRequest req{detail::unrows(out, 32)};
        return {FinalizeData{inputs, blinds, req}, req};
    }
    // client.go Client.Finalize (base mode)
    List Finalize(const FinalizeData &f, const Evaluation &e) const {
        if (mode_ != BaseMode) throw ErrModeNotServed();
        const size_t n = f.inputs.size();
        if (e.Elements.size() != n) throw ErrBatchSize();
        Bytes b = detail::rows(f.blinds, n), ev = detail::rows(e.Elements, n), out(64 * n), ok(n);
        const detail::Ragged in(f.inputs);
        detail::check(circl_hip_oprf_finalize(in.blob(), in.offs(), b.data(), ev.data(), out.data(), ok.data(), n, device_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw ErrInvalidElement();
        }
        List r = detail::unrows(out, 64);
        detail::wipe(out);
        return r;
    }

private:
    Mode mode_;
    int device_;
};

// what Server and VerifiableServer share: one key for every batch
class ServerBase {
public:
    PublicKey Public() const { return key_.Public(); }
    // server.go FullEvaluate
    List FullEvaluate(const List &inputs) const {
        const size_t n = inputs.size();
        Bytes out(64 * n), ok(n);
        const detail::Ragged in(inputs);
        detail::check(circl_hip_oprf_full_evaluate(mode_, key_.k.data(), 0, in.blob(), in.offs(), out.data(), ok.data(), n, device_));
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            if (!detail::scalar_usable(key_.k)) throw ErrInvalidScalar();
            throw ErrInvalidInput();
        }
        List r = detail::unrows(out, 64);
        detail::wipe(out);
        return r;
    }
    ~ServerBase() { detail::wipe(key_.k); }

protected:
    ServerBase(Mode mode, PrivateKey key, int device) : mode_(mode), key_(std::move(key)), device_(device) {}
    Mode mode_;
    PrivateKey key_;
    int device_;
};

class Server : public ServerBase {
public:
    explicit Server(PrivateKey key, int device = 0) : ServerBase(BaseMode, std::move(key), device) {}
    // server.go Server.Evaluate
    Evaluation Evaluate(const EvaluationRequest &req) const {
        const size_t n = req.Elements.size();
        Bytes el = detail::rows(req.Elements, n), out(32 * n), ok(n);
        detail::check(circl_hip_oprf_evaluate(key_.k.data(), 0, el.data(), out.data(), ok.data(), n, device_));
        if (!detail::all_ok(ok)) {
            if (!detail::scalar_usable(key_.k)) throw ErrInvalidScalar();
            throw ErrInvalidElement();
        }
        return Evaluation{detail::unrows(out, 32)};
    }
};

namespace detail {
inline Bytes context_string(Mode mode) {
    const std::string s = std::string("OPRFV1-") + char(mode) + "-ristretto255-SHA512";
    return Bytes(s.begin(), s.end());
}
// one request of n element pairs proven under k (kA = k G): the proof, or ErrInvalidElement / ErrInvalidScalar
inline Bytes prove(Mode mode, const Bytes &k, const Bytes &kA, const Bytes &B, const Bytes &kB, size_t n, const Bytes &r, int device) {
    if (r.size() != 32) throw ErrInvalidScalar();
    const uint64_t off[2] = {0, n};
    const Bytes ctx = context_string(mode);
    Bytes proof(64), ok(1);
    check(circl_hip_dleq_prove(k.data(), 0, kA.data(), 0, B.data(), kB.data(), off, r.data(), ctx.data(), ctx.size(), CIRCL_HIP_DLEQ_NO_IDENTITY, proof.data(),
                               ok.data(), 1, device));
    if (!ok[0]) {
        if (!scalar_usable(k) || !scalar_usable(r)) throw ErrInvalidScalar();
        throw ErrInvalidElement();
    }
    return proof;
}
inline bool verify(Mode mode, const Bytes &kA, const Bytes &B, const Bytes &kB, size_t n, const Bytes &proof, int device) {
    if (proof.size() != 64 || kA.size() != 32) return false;
    const uint64_t off[2] = {0, n};
    const Bytes ctx = context_string(mode);
    Bytes ok(1);
    check(circl_hip_dleq_verify(kA.data(), 0, B.data(), kB.data(), off, proof.data(), ctx.data(), ctx.size(), CIRCL_HIP_DLEQ_NO_IDENTITY, ok.data(), 1, device));
    return ok[0] != 0;
}
// base-mode evaluation of n elements under the scalar k
inline Bytes evaluate(const Bytes &k, const Bytes &el, size_t n, int device) {
    Bytes out(32 * n), ok(n);
    check(circl_hip_oprf_evaluate(k.data(), 0, el.data(), out.data(), ok.data(), n, device));
    if (!all_ok(ok)) {
        if (!scalar_usable(k)) throw ErrInvalidScalar();
        throw ErrInvalidElement();
    }
    return out;
}
}  // namespace detail

// server.go VerifiableServer: Evaluate = the base evaluation and one proof for the request
class VerifiableServer : public ServerBase {
public:
    explicit VerifiableServer(PrivateKey key, int device = 0) : ServerBase(VerifiableMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &req, const Bytes &r) const {
        const size_t n = req.Elements.size();
        if (n == 0) throw ErrInvalidInput();
        const Bytes el = detail::rows(req.Elements, n), out = detail::evaluate(key_.k, el, n, device_);
        return Evaluation{detail::unrows(out, 32), detail::prove(VerifiableMode, key_.k, key_.pub, el, out, n, r, device_)};
    }
};

// server.go PartialObliviousServer: the key is tweaked by the info; the proof is under t = sk + m with the roles of the elements swapped
class PartialObliviousServer : public ServerBase {
public:
    explicit PartialObliviousServer(PrivateKey key, int device = 0) : ServerBase(PartialObliviousMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &req, const Bytes &info, const Bytes &r) const {
        const size_t n = req.Elements.size();
        if (n == 0) throw ErrInvalidInput();
        const detail::Ragged inf(List{info});
        Bytes t(32), tinv(32), tg(32), ok(1);
        detail::check(circl_hip_oprf_poprf_tweak(key_.k.data(), 0, nullptr, 0, inf.blob(), inf.offs(), t.data(), tinv.data(), tg.data(), ok.data(), 1, device_));
        if (!ok[0]) throw ErrInvalidInput();  // ErrInverseZero, an info over 65535 bytes, an unusable key
        const Bytes el = detail::rows(req.Elements, n), out = detail::evaluate(tinv, el, n, device_);
        Evaluation e{detail::unrows(out, 32), detail::prove(PartialObliviousMode, t, tg, out, el, n, r, device_)};
        detail::wipe(t);
        detail::wipe(tinv);
        return e;
    }
    List FullEvaluate(const List &inputs, const Bytes &info) const {
        const size_t n = inputs.size();
        Bytes out(64 * n), ok(n);
        const detail::Ragged in(inputs), inf(List(n, info));
        detail::check(circl_hip_oprf_poprf_full_evaluate(key_.k.data(), 0, in.blob(), in.offs(), inf.blob(), inf.offs(), out.data(), ok.data(), n, device_));
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw ErrInvalidInput();
        }
        List r = detail::unrows(out, 64);
        detail::wipe(out);
        return r;
    }

private:
    using ServerBase::FullEvaluate;  // (the form without an info is not POPRF's)
};

// client.go VerifiableClient: Finalize verifies the proof first; nothing is returned unless it holds
class VerifiableClient : public Client {
public:
    explicit VerifiableClient(PublicKey pkS, int device = 0) : Client(VerifiableMode, device), pk_(std::move(pkS)), dev_(device) {}
    List Finalize(const FinalizeData &f, const Evaluation &e) const {
        const size_t n = f.inputs.size();
        if (n == 0 || e.Elements.size() != n || f.evalReq.Elements.size() != n) throw ErrBatchSize();
        const Bytes bl = detail::rows(f.evalReq.Elements, n), ev = detail::rows(e.Elements, n);
        if (!detail::verify(VerifiableMode, pk_.e, bl, ev, n, e.Proof, dev_)) throw ErrInvalidProof();
        return Client(BaseMode, dev_).Finalize(f, e);  // the same hash as base mode
    }

private:
    PublicKey pk_;
    int dev_;
};

// client.go PartialObliviousClient
class PartialObliviousClient : public Client {
public:
    explicit PartialObliviousClient(PublicKey pkS, int device = 0) : Client(PartialObliviousMode, device), pk_(std::move(pkS)), dev_(device) {}
    List Finalize(const FinalizeData &f, const Evaluation &e, const Bytes &info) const {
        const size_t n = f.inputs.size();
        if (n == 0 || e.Elements.size() != n || f.evalReq.Elements.size() != n) throw ErrBatchSize();
        if (pk_.e.size() != 32) throw ErrInvalidElement();
        const detail::Ragged one(List{info});
        Bytes tweaked(32), ok1(1);
        detail::check(circl_hip_oprf_poprf_tweak(nullptr, 0, pk_.e.data(), 0, one.blob(), one.offs(), nullptr, nullptr, tweaked.data(), ok1.data(), 1, dev_));
        if (!ok1[0]) throw ErrInvalidInput();  // ErrInvalidInfo
        const Bytes bl = detail::rows(f.evalReq.Elements, n), ev = detail::rows(e.Elements, n);
        if (!detail::verify(PartialObliviousMode, tweaked, ev, bl, n, e.Proof, dev_)) throw ErrInvalidProof();
        Bytes b = detail::rows(f.blinds, n), out(64 * n), ok(n);
        const detail::Ragged in(f.inputs), inf(List(n, info));
        detail::check(circl_hip_oprf_poprf_finalize(in.blob(), in.offs(), inf.blob(), inf.offs(), b.data(), ev.data(), out.data(), ok.data(), n, dev_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw ErrInvalidElement();
        }
        List r = detail::unrows(out, 64);
        detail::wipe(out);
        return r;
    }

private:
    PublicKey pk_;
    int dev_;
};

}  // namespace oprf
}  // namespace circl
