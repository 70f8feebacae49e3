// tests/oprf_test.cpp -- the C++ mirror of the ristretto255 group and base-mode OPRF (include/circl/oprf.hpp) on the GPU: DeriveKey ->
// Client.DeterministicBlind -> Server.Evaluate -> Client.Finalize for a batch of 65 whose item 0 is the first RFC 9497 vector of
// ristretto255-SHA512 in base mode (blinded element, evaluated element and output are checked against the published values), and the
// same outputs from Server.FullEvaluate; VerifiableServer.FullEvaluate on the mode-1 vector; the public keys of modes 1 and 2; the
// group level (MulGen, Mul and its inverse, the two hashes); a zero blind, an element that does not decode and the verifiable
// Finalize, which throw.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/oprf.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace circl;
using oprf::Bytes;
using oprf::List;

template <class E, class F> static bool throws(F &&f) {
    try { f(); } catch (const E &) { return true; }
    return false;
}

static Bytes hex(const char *s) {
    Bytes b;
    for (; s[0] && s[1]; s += 2) {
        unsigned v;
        sscanf(s, "%2x", &v);
        b.push_back((uint8_t)v);
    }
    return b;
}

static Bytes pattern(size_t len, unsigned seed) {
    Bytes b(len);
    for (size_t i = 0; i < len; i++) b[i] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    return b;
}

static Bytes small_scalar(unsigned seed) {  // 31 random bytes: below the group order, not zero
    Bytes b = pattern(32, seed);
    b[0] |= 1;
    b[31] = 0;
    return b;
}

int main() {
    const Bytes seed(32, 0xa3), info = hex("74657374206b6579");
    // keys of the three modes (RFC 9497 A.1)
    const oprf::PrivateKey k0 = oprf::DeriveKey(oprf::BaseMode, seed, info), k1 = oprf::DeriveKey(oprf::VerifiableMode, seed, info),
                           k2 = oprf::DeriveKey(oprf::PartialObliviousMode, seed, info);
    CHECK(k0.MarshalBinary() == hex("5ebcea5ee37023ccb9fc2d2019f9d7737be85591ae8652ffa9ef0f4d37063b0e"));
    CHECK(k1.MarshalBinary() == hex("e6f73f344b79b379f1a0dd37e07ff62e38d9f71345ce62ae3a9bc60b04ccd909"));
    CHECK(k1.Public().MarshalBinary() == hex("c803e2cc6b05fc15064549b5920659ca4a77b2cca6f04f6b357009335476ad4e"));
    CHECK(k2.Public().MarshalBinary() == hex("c647bef38497bc6ec077c22af65b696efa43bff3b4a1975a3e8e0a1c5a79d631"));

    const size_t n = 65;
    List inputs, blinds;
    for (size_t i = 0; i < n; i++) {
        inputs.push_back(i == 0 ? hex("00") : pattern((i * 5) % 90, 100 + i));
        blinds.push_back(i == 0 ? hex("64d37aed22a27f5191de1c1d69fadb899d8862b58eb4220029e036ec4c1f6706") : small_scalar(300 + i));
    }
    const oprf::Client client(oprf::BaseMode);
    const oprf::Server server(k0);
    auto b = client.DeterministicBlind(inputs, blinds);
    CHECK(b.second.Elements.size() == n);
    CHECK(b.second.Elements[0] == hex("609a0ae68c15a3cf6903766461307e5c8bb2f95e7e6550e1ffa2dc99e412803c"));
    const oprf::Evaluation ev = server.Evaluate(b.second);
    CHECK(ev.Elements[0] == hex("7ec6578ae5120958eb2db1745758ff379e77cb64fe77b0b2d8cc917ea0869c7e"));
    const List out = client.Finalize(b.first, ev), full = server.FullEvaluate(inputs);
    CHECK(out[0] == hex("527759c3d9366f277d8c6020418d96bb393ba2afb20ff90df23fb7708264e2f3ab9135e3bd69955851de4b1f9fe8a0973396719b7912ba9ee8aa7d0b5e24bcf6"));
    CHECK(out.size() == n && out == full);
    for (size_t i = 1; i < n; i++) CHECK(out[i].size() == 64 && out[i] != out[0]);

    const oprf::VerifiableServer vserver(k1);
    CHECK(vserver.FullEvaluate({hex("00")})[0] ==
          hex("b58cfbe118e0cb94d79b5fd6a6dafb98764dff49c14e1770b566e42402da1a7da4d8527693914139caee5bd03903af43a491351d23b430948dd50cde10d32b3c"));
    CHECK(throws<oprf::ErrModeNotServed>([&] { oprf::Client(oprf::VerifiableMode).Finalize(b.first, ev); }));

    // the group level: 15 B, k (k^-1 P) = P, a public key is sk B, the hashes answer per item
    Bytes fifteen(32, 0);
    fifteen[0] = 15;
    auto g15 = group::Ristretto255::MulGen({fifteen});
    CHECK(g15.second[0] == 1 && g15.first[0] == hex("e0c418f7c8d9c4cdd7395b93ea124f3ad99021bb681dfc3302a9d99a2e53e64e"));
    CHECK(group::Ristretto255::MulGen({k1.MarshalBinary()}).first[0] == k1.Public().MarshalBinary());
    auto unblinded = group::Ristretto255::MulInverse(blinds, b.second.Elements);
    const Bytes dst = hex("48617368546f47726f75702d4f50524656312d002d72697374726574746f3235352d534841353132");  // "HashToGroup-" || the mode-0 context
    CHECK(unblinded.first == group::Ristretto255::HashToElement(inputs, dst));
    auto shared = group::Ristretto255::Mul({k0.MarshalBinary()}, b.second.Elements);  // one scalar for the batch
    CHECK(shared.first == ev.Elements);
    const List scalars = group::Ristretto255::HashToScalar(inputs, dst);
    CHECK(scalars.size() == n && scalars[1] != scalars[2] && (scalars[1][31] & 0xf0) == 0);

    // what the protocol refuses
    List bad_blinds = blinds;
    bad_blinds[33] = Bytes(32, 0);
    CHECK(throws<oprf::ErrInvalidScalar>([&] { client.DeterministicBlind(inputs, bad_blinds); }));
    oprf::EvaluationRequest bad_req = b.second;
    bad_req.Elements[64] = hex("0100000000000000000000000000000000000000000000000000000000000000");  // a negative s
    CHECK(throws<oprf::ErrInvalidElement>([&] { server.Evaluate(bad_req); }));
    bad_req.Elements[64] = hex("edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f");  // s = p: the reference would reduce it
    CHECK(throws<oprf::ErrInvalidElement>([&] { server.Evaluate(bad_req); }));
    oprf::Evaluation bad_ev = ev;
    bad_ev.Elements[1] = Bytes(32, 0);  // the identity
    CHECK(throws<oprf::ErrInvalidElement>([&] { client.Finalize(b.first, bad_ev); }));
    List long_inputs = {Bytes(65536, 7)};
    CHECK(throws<oprf::ErrInvalidInput>([&] { client.DeterministicBlind(long_inputs, {blinds[0]}); }));
    CHECK(throws<oprf::ErrInvalidInput>([&] { server.FullEvaluate(long_inputs); }));
    puts("OK");
    return 0;
}
