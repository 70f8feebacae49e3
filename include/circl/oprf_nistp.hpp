// circl/oprf_nistp.hpp -- the NIST P-256 / P-384 groups and base-mode OPRF on them (suites P256-SHA256, P384-SHA384) on top of the HIP
// batch engine, shaped like circl/oprf.hpp and so like the reference's group.P256 / group.P384 (group/short.go) and oprf package, over
// batches.  Everything is a template over the curve (nistp::P256, nistp::P384):
//
//   nistp::Group<C>::HashToElement(msgs, dst) / HashToElementNonUniform / HashToScalar     -> n encodings
//   nistp::Group<C>::Mul(scalars, elems) / MulGen(scalars) / MulInverse                     -> {n encodings, ok}; one scalar serves the batch
//   nistp::DeriveKey<C>(mode, seed, info)                                                   -> PrivateKey (carries its public key)
//   nistp::Client<C>(mode).DeterministicBlind(inputs, blinds)                               -> {FinalizeData, EvaluationRequest}
//   nistp::Server<C>(key).Evaluate(request)                                                 -> Evaluation           (base mode)
//   nistp::Client<C>(mode).Finalize(finalizeData, evaluation)                               -> n outputs of 32 / 48 bytes (base mode)
//   nistp::Server<C>(key).FullEvaluate(inputs) / nistp::VerifiableServer<C>(key).FullEvaluate(inputs)   -> n outputs
// Scalars, keys and blinds are big-endian, 32 / 48 bytes; elements are SEC 1 COMPRESSED, 33 / 49 bytes, and the identity is the all-zero
// row (include/circl_hip.h states this one difference from the reference).  Errors are circl/oprf.hpp's.  Link with -lcirclhip.
//
// The verifiable modes, with their DLEQ proofs (circl_hip_nistp_dleq_*, circl_hip_oprf_nistp_poprf_*), are the four classes of
// namespace nistp::proofs, shaped like those of circl/oprf.hpp:
//   nistp::proofs::VerifiableServer<C>(key).Evaluate(request, r) / PartialObliviousServer<C>(key).Evaluate(request, info, r)  -> Evaluation with its proof
//   nistp::proofs::VerifiableClient<C>(pkS).Finalize(finalizeData, evaluation) / PartialObliviousClient<C>(pkS).Finalize(.., info) -> n outputs
// A proof is c || s, 64 / 96 bytes; r is the proof randomness, drawn by the caller.  A proof that does not verify throws
// oprf::ErrInvalidProof and no output leaves the call.  They live in a namespace of their own because nistp::VerifiableServer<C> and
// nistp::Client<C> below are the proof-free classes of the first NIST release: their Evaluate / Finalize in a verifiable mode keep
// throwing oprf::ErrModeNotServed, which callers (and tests/oprf_nistp_test.cpp) rely on.
#pragma once
#include "oprf.hpp"

namespace circl {
namespace nistp {
using oprf::Bytes;
using oprf::List;
using oprf::Mode;

struct P256 {
    static constexpr int CURVE = CIRCL_HIP_P256;
    static constexpr size_t Ns = 32, Ne = 33, Nh = 32;
};
struct P384 {
    static constexpr int CURVE = CIRCL_HIP_P384;
    static constexpr size_t Ns = 48, Ne = 49, Nh = 48;
};

namespace detail {
using oprf::detail::all_ok;
using oprf::detail::check;
using oprf::detail::Ragged;
using oprf::detail::unrows;
using oprf::detail::wipe;
// n rows of `width` bytes, contiguous
inline Bytes rows(const List &l, size_t n, size_t width) {
    if (l.size() != n) throw oprf::ErrBatchSize();
    Bytes r;
    for (auto &k : l) {
        if (k.size() != width) throw oprf::ErrBatchSize();
        r.insert(r.end(), k.begin(), k.end());
    }
    return r;
}
inline bool nonzero(const Bytes &k) {
    for (uint8_t b : k)
        if (b) return true;
    return false;
}
}  // namespace detail

// group.P256 / group.P384 over batches: elements and scalars are their encodings
template <class C>
struct Group {
    static List HashToElement(const List &msgs, const Bytes &dst, bool nonuniform = false, int device = 0) {
        const detail::Ragged m(msgs);
        Bytes out(C::Ne * msgs.size());
        detail::check(circl_hip_nistp_hash_to_group(C::CURVE, m.blob(), m.offs(), dst.data(), dst.size(), nonuniform ? CIRCL_HIP_NISTP_NONUNIFORM : 0, out.data(),
                                                    msgs.size(), device));
        return detail::unrows(out, C::Ne);
    }
    static List HashToElementNonUniform(const List &msgs, const Bytes &dst, int device = 0) { return HashToElement(msgs, dst, true, device); }
    static List HashToScalar(const List &msgs, const Bytes &dst, int device = 0) {
        const detail::Ragged m(msgs);
        Bytes out(C::Ns * msgs.size());
        detail::check(circl_hip_nistp_hash_to_scalar(C::CURVE, m.blob(), m.offs(), dst.data(), dst.size(), out.data(), msgs.size(), device));
        return detail::unrows(out, C::Ns);
    }
    // scalars: n of them, or one for the batch; elems empty: the generator (then n = scalars.size()).  -> {n encodings, ok}
    static std::pair<List, Bytes> Mul(const List &scalars, const List &elems, bool invert = false, int device = 0) {
        const size_t n = elems.empty() ? scalars.size() : elems.size();
        const bool shared = scalars.size() == 1 && n != 1;
        Bytes sc = detail::rows(scalars, shared ? 1 : n, C::Ns), el = elems.empty() ? Bytes() : detail::rows(elems, n, C::Ne), out(C::Ne * n), ok(n);
        detail::check(circl_hip_nistp_scalar_mult(C::CURVE, sc.data(), shared ? 0 : C::Ns, elems.empty() ? nullptr : el.data(), invert ? CIRCL_HIP_NISTP_INVERT : 0,
                                                  out.data(), ok.data(), n, device));
        detail::wipe(sc);
        return {detail::unrows(out, C::Ne), ok};
    }
    static std::pair<List, Bytes> MulGen(const List &scalars, int device = 0) { return Mul(scalars, {}, false, device); }
    static std::pair<List, Bytes> MulInverse(const List &scalars, const List &elems, int device = 0) { return Mul(scalars, elems, true, device); }
};

using oprf::Evaluation;
using oprf::EvaluationRequest;
using oprf::FinalizeData;
using oprf::PrivateKey;
using oprf::PublicKey;

// oprf.DeriveKey(suite, mode, seed, info) for n (seed, info) pairs
template <class C>
inline std::vector<PrivateKey> DeriveKeys(Mode mode, const List &seeds, const List &infos, int device = 0) {
    const size_t n = seeds.size();
    if (infos.size() != n) throw oprf::ErrBatchSize();
    Bytes s = detail::rows(seeds, n, 32), sk(C::Ns * n), pk(C::Ne * n), ok(n);
    const detail::Ragged info(infos);
    detail::check(circl_hip_oprf_nistp_derive_keypair(C::CURVE, mode, s.data(), info.blob(), info.offs(), sk.data(), pk.data(), ok.data(), n, device));
    detail::wipe(s);
    if (!detail::all_ok(ok)) throw oprf::ErrInvalidInput();
    std::vector<PrivateKey> keys(n);
    for (size_t i = 0; i < n; i++)
        keys[i] = PrivateKey{Bytes(sk.begin() + C::Ns * i, sk.begin() + C::Ns * (i + 1)), Bytes(pk.begin() + C::Ne * i, pk.begin() + C::Ne * (i + 1))};
    detail::wipe(sk);
    return keys;
}
template <class C>
inline PrivateKey DeriveKey(Mode mode, const Bytes &seed, const Bytes &info, int device = 0) {
    return DeriveKeys<C>(mode, {seed}, {info}, device)[0];
}

template <class C>
class Client {
public:
    explicit Client(Mode mode, int device = 0) : mode_(mode), device_(device) {}
    // client.go DeterministicBlind
    std::pair<FinalizeData, EvaluationRequest> DeterministicBlind(const List &inputs, const List &blinds) const {
        const size_t n = inputs.size();
        if (n == 0) throw oprf::ErrInvalidInput();
        Bytes b = detail::rows(blinds, n, C::Ns), out(C::Ne * n), ok(n);
        const detail::Ragged in(inputs);
        detail::check(circl_hip_oprf_nistp_blind(C::CURVE, mode_, in.blob(), in.offs(), b.data(), out.data(), ok.data(), n, device_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            for (size_t i = 0; i < n; i++)
                if (!ok[i] && inputs[i].size() <= 0xffff) throw oprf::ErrInvalidScalar();  // (an identity hashed point aside: a zero or non-canonical blind)
            throw oprf::ErrInvalidInput();
        }
        EvaluationRequest req{detail::unrows(out, C::Ne)};
        return {FinalizeData{inputs, blinds, req}, req};
    }
    // client.go Client.Finalize (base mode)
    List Finalize(const FinalizeData &f, const Evaluation &e) const {
        if (mode_ != oprf::BaseMode) throw oprf::ErrModeNotServed();
        const size_t n = f.inputs.size();
        if (e.Elements.size() != n) throw oprf::ErrBatchSize();
        Bytes b = detail::rows(f.blinds, n, C::Ns), ev = detail::rows(e.Elements, n, C::Ne), out(C::Nh * n), ok(n);
        const detail::Ragged in(f.inputs);
        detail::check(circl_hip_oprf_nistp_finalize(C::CURVE, in.blob(), in.offs(), b.data(), ev.data(), out.data(), ok.data(), n, device_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw oprf::ErrInvalidElement();
        }
        List r = detail::unrows(out, C::Nh);
        detail::wipe(out);
        return r;
    }

private:
    Mode mode_;
    int device_;
};

// what Server and VerifiableServer share: one key for every batch
template <class C>
class ServerBase {
public:
    PublicKey Public() const { return key_.Public(); }
    // server.go FullEvaluate
    List FullEvaluate(const List &inputs) const {
        const size_t n = inputs.size();
        Bytes out(C::Nh * n), ok(n);
        const detail::Ragged in(inputs);
        detail::check(circl_hip_oprf_nistp_full_evaluate(C::CURVE, mode_, key_.k.data(), 0, in.blob(), in.offs(), out.data(), ok.data(), n, device_));
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            for (auto &x : inputs)
                if (x.size() > 0xffff) throw oprf::ErrInvalidInput();
            throw oprf::ErrInvalidScalar();
        }
        List r = detail::unrows(out, C::Nh);
        detail::wipe(out);
        return r;
    }
    ~ServerBase() { detail::wipe(key_.k); }

protected:
    ServerBase(Mode mode, PrivateKey key, int device) : mode_(mode), key_(std::move(key)), device_(device) {
        if (key_.k.size() != C::Ns) throw oprf::ErrInvalidScalar();
    }
    Mode mode_;
    PrivateKey key_;
    int device_;
};

template <class C>
class Server : public ServerBase<C> {
public:
    explicit Server(PrivateKey key, int device = 0) : ServerBase<C>(oprf::BaseMode, std::move(key), device) {}
    // server.go Server.Evaluate
    Evaluation Evaluate(const EvaluationRequest &req) const {
        const size_t n = req.Elements.size();
        Bytes el = detail::rows(req.Elements, n, C::Ne), out(C::Ne * n), ok(n), one(C::Ne * 1), ok1(1);
        detail::check(circl_hip_oprf_nistp_evaluate(C::CURVE, this->key_.k.data(), 0, el.data(), out.data(), ok.data(), n, this->device_));
        if (!detail::all_ok(ok)) {
            // whose fault: the key multiplies the generator exactly when it is canonical (zero gives the identity, which is no element here)
            detail::check(circl_hip_nistp_scalar_mult(C::CURVE, this->key_.k.data(), 0, nullptr, 0, one.data(), ok1.data(), 1, this->device_));
            if (!ok1[0] || !detail::nonzero(this->key_.k)) throw oprf::ErrInvalidScalar();
            throw oprf::ErrInvalidElement();
        }
        return Evaluation{detail::unrows(out, C::Ne)};
    }
};

// server.go VerifiableServer without the proof: FullEvaluate is served; Evaluate with its DLEQ proof is proofs::VerifiableServer's
template <class C>
class VerifiableServer : public ServerBase<C> {
public:
    explicit VerifiableServer(PrivateKey key, int device = 0) : ServerBase<C>(oprf::VerifiableMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &, const Bytes &) const { throw oprf::ErrModeNotServed(); }
};

namespace detail {
template <class C>
inline Bytes context_string(Mode mode) {
    const std::string s = std::string("OPRFV1-") + char(mode) + (C::CURVE == CIRCL_HIP_P256 ? "-P256-SHA256" : "-P384-SHA384");
    return Bytes(s.begin(), s.end());
}
// the key multiplies the generator exactly when it is canonical; zero is no key
template <class C>
inline bool scalar_usable(const Bytes &k, int device) {
    if (k.size() != C::Ns || !nonzero(k)) return false;
    Bytes one(C::Ne), ok(1);
    check(circl_hip_nistp_scalar_mult(C::CURVE, k.data(), 0, nullptr, 0, one.data(), ok.data(), 1, device));
    return ok[0] != 0;
}
// one request of n element pairs proven under k (kA = k G): the proof, or ErrInvalidElement / ErrInvalidScalar
template <class C>
inline Bytes prove(Mode mode, const Bytes &k, const Bytes &kA, const Bytes &B, const Bytes &kB, size_t n, const Bytes &r, int device) {
    if (r.size() != C::Ns || k.size() != C::Ns || kA.size() != C::Ne) throw oprf::ErrInvalidScalar();
    const uint64_t off[2] = {0, n};
    const Bytes ctx = context_string<C>(mode);
    Bytes proof(2 * C::Ns), ok(1);
    check(circl_hip_nistp_dleq_prove(C::CURVE, k.data(), 0, kA.data(), 0, B.data(), kB.data(), off, r.data(), ctx.data(), ctx.size(), CIRCL_HIP_DLEQ_NO_IDENTITY,
                                     proof.data(), ok.data(), 1, device));
    if (!ok[0]) {
        if (!scalar_usable<C>(k, device) || !scalar_usable<C>(r, device)) throw oprf::ErrInvalidScalar();
        throw oprf::ErrInvalidElement();
    }
    return proof;
}
template <class C>
inline bool verify(Mode mode, const Bytes &kA, const Bytes &B, const Bytes &kB, size_t n, const Bytes &proof, int device) {
    if (proof.size() != 2 * C::Ns || kA.size() != C::Ne) return false;
    const uint64_t off[2] = {0, n};
    const Bytes ctx = context_string<C>(mode);
    Bytes ok(1);
    check(circl_hip_nistp_dleq_verify(C::CURVE, kA.data(), 0, B.data(), kB.data(), off, proof.data(), ctx.data(), ctx.size(), CIRCL_HIP_DLEQ_NO_IDENTITY, ok.data(), 1,
                                      device));
    return ok[0] != 0;
}
// base-mode evaluation of n elements under the scalar k
template <class C>
inline Bytes evaluate(const Bytes &k, const Bytes &el, size_t n, int device) {
    Bytes out(C::Ne * n), ok(n);
    check(circl_hip_oprf_nistp_evaluate(C::CURVE, k.data(), 0, el.data(), out.data(), ok.data(), n, device));
    if (!all_ok(ok)) {
        if (!scalar_usable<C>(k, device)) throw oprf::ErrInvalidScalar();
        throw oprf::ErrInvalidElement();
    }
    return out;
}
}  // namespace detail

// ---- the verifiable modes with their proofs (see the head of this file for why they have a namespace of their own) -----------------
namespace proofs {

// server.go VerifiableServer: Evaluate = the base evaluation and one proof for the request
template <class C>
class VerifiableServer : public ServerBase<C> {
public:
    explicit VerifiableServer(PrivateKey key, int device = 0) : ServerBase<C>(oprf::VerifiableMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &req, const Bytes &r) const {
        const size_t n = req.Elements.size();
        if (n == 0) throw oprf::ErrInvalidInput();
        const Bytes el = detail::rows(req.Elements, n, C::Ne), out = detail::evaluate<C>(this->key_.k, el, n, this->device_);
        return Evaluation{detail::unrows(out, C::Ne), detail::prove<C>(oprf::VerifiableMode, this->key_.k, this->key_.pub, el, out, n, r, this->device_)};
    }
};

// server.go PartialObliviousServer: the key is tweaked by the info; the proof is under t = sk + m with the roles of the elements swapped
template <class C>
class PartialObliviousServer : public ServerBase<C> {
public:
    explicit PartialObliviousServer(PrivateKey key, int device = 0) : ServerBase<C>(oprf::PartialObliviousMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &req, const Bytes &info, const Bytes &r) const {
        const size_t n = req.Elements.size();
        if (n == 0) throw oprf::ErrInvalidInput();
        const detail::Ragged inf(List{info});
        Bytes t(C::Ns), tinv(C::Ns), tg(C::Ne), ok(1);
        detail::check(circl_hip_oprf_nistp_poprf_tweak(C::CURVE, this->key_.k.data(), 0, nullptr, 0, inf.blob(), inf.offs(), t.data(), tinv.data(), tg.data(), ok.data(),
                                                       1, this->device_));
        if (!ok[0]) throw oprf::ErrInvalidInput();  // ErrInverseZero, an info over 65535 bytes, an unusable key
        const Bytes el = detail::rows(req.Elements, n, C::Ne), out = detail::evaluate<C>(tinv, el, n, this->device_);
        Evaluation e{detail::unrows(out, C::Ne), detail::prove<C>(oprf::PartialObliviousMode, t, tg, out, el, n, r, this->device_)};
        detail::wipe(t);
        detail::wipe(tinv);
        return e;
    }
    List FullEvaluate(const List &inputs, const Bytes &info) const {
        const size_t n = inputs.size();
        Bytes out(C::Nh * n), ok(n);
        const detail::Ragged in(inputs), inf(List(n, info));
        detail::check(circl_hip_oprf_nistp_poprf_full_evaluate(C::CURVE, this->key_.k.data(), 0, in.blob(), in.offs(), inf.blob(), inf.offs(), out.data(), ok.data(), n,
                                                               this->device_));
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw oprf::ErrInvalidInput();
        }
        List r = detail::unrows(out, C::Nh);
        detail::wipe(out);
        return r;
    }

private:
    using ServerBase<C>::FullEvaluate;  // (the form without an info is not POPRF's)
};

// client.go VerifiableClient: Finalize verifies the proof first; nothing is returned unless it holds
template <class C>
class VerifiableClient : public Client<C> {
public:
    explicit VerifiableClient(PublicKey pkS, int device = 0) : Client<C>(oprf::VerifiableMode, device), pk_(std::move(pkS)), dev_(device) {}
    List Finalize(const FinalizeData &f, const Evaluation &e) const {
        const size_t n = f.inputs.size();
        if (n == 0 || e.Elements.size() != n || f.evalReq.Elements.size() != n) throw oprf::ErrBatchSize();
        const Bytes bl = detail::rows(f.evalReq.Elements, n, C::Ne), ev = detail::rows(e.Elements, n, C::Ne);
        if (!detail::verify<C>(oprf::VerifiableMode, pk_.e, bl, ev, n, e.Proof, dev_)) throw oprf::ErrInvalidProof();
        return Client<C>(oprf::BaseMode, dev_).Finalize(f, e);  // the same hash as base mode
    }

private:
    PublicKey pk_;
    int dev_;
};

// client.go PartialObliviousClient
template <class C>
class PartialObliviousClient : public Client<C> {
public:
    explicit PartialObliviousClient(PublicKey pkS, int device = 0) : Client<C>(oprf::PartialObliviousMode, device), pk_(std::move(pkS)), dev_(device) {}
    List Finalize(const FinalizeData &f, const Evaluation &e, const Bytes &info) const {
        const size_t n = f.inputs.size();
        if (n == 0 || e.Elements.size() != n || f.evalReq.Elements.size() != n) throw oprf::ErrBatchSize();
        if (pk_.e.size() != C::Ne) throw oprf::ErrInvalidElement();
        const detail::Ragged one(List{info});
        Bytes tweaked(C::Ne), ok1(1);
        detail::check(circl_hip_oprf_nistp_poprf_tweak(C::CURVE, nullptr, 0, pk_.e.data(), 0, one.blob(), one.offs(), nullptr, nullptr, tweaked.data(), ok1.data(), 1,
                                                       dev_));
        if (!ok1[0]) throw oprf::ErrInvalidInput();  // ErrInvalidInfo
        const Bytes bl = detail::rows(f.evalReq.Elements, n, C::Ne), ev = detail::rows(e.Elements, n, C::Ne);
        if (!detail::verify<C>(oprf::PartialObliviousMode, tweaked, ev, bl, n, e.Proof, dev_)) throw oprf::ErrInvalidProof();
        Bytes b = detail::rows(f.blinds, n, C::Ns), out(C::Nh * n), ok(n);
        const detail::Ragged in(f.inputs), inf(List(n, info));
        detail::check(circl_hip_oprf_nistp_poprf_finalize(C::CURVE, in.blob(), in.offs(), inf.blob(), inf.offs(), b.data(), ev.data(), out.data(), ok.data(), n, dev_));
        detail::wipe(b);
        if (!detail::all_ok(ok)) {
            detail::wipe(out);
            throw oprf::ErrInvalidElement();
        }
        List r = detail::unrows(out, C::Nh);
        detail::wipe(out);
        return r;
    }

private:
    PublicKey pk_;
    int dev_;
};

}  // namespace proofs

}  // namespace nistp
}  // namespace circl
