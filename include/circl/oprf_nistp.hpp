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
// row (include/circl_hip.h states this one difference from the reference).  The proofs of the verifiable modes are not served on these
// curves: their Evaluate / Finalize throw oprf::ErrModeNotServed.  Errors are circl/oprf.hpp's.  Link with -lcirclhip.
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

// server.go VerifiableServer: FullEvaluate is served; Evaluate needs the DLEQ proof, which is not served on these curves
template <class C>
class VerifiableServer : public ServerBase<C> {
public:
    explicit VerifiableServer(PrivateKey key, int device = 0) : ServerBase<C>(oprf::VerifiableMode, std::move(key), device) {}
    Evaluation Evaluate(const EvaluationRequest &, const Bytes &) const { throw oprf::ErrModeNotServed(); }
};

}  // namespace nistp
}  // namespace circl
