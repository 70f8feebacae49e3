// tests/oprf_nistp_test.cpp -- the C++ mirror of the P-256 / P-384 groups and base-mode OPRF (include/circl/oprf_nistp.hpp) on the GPU, per
// curve: DeriveKey -> Client.DeterministicBlind -> Server.Evaluate -> Client.Finalize for a batch of 65 whose item 0 is the first RFC 9497
// vector of the suite in base mode (key, blinded element, evaluated element and output are checked against the published values), and the
// same outputs from Server.FullEvaluate; VerifiableServer.FullEvaluate on the mode-1 vector; the public keys of modes 1 and 2; the group
// level (MulGen, Mul and its inverse, the hashes); a zero blind, an element that does not decode, the identity and the verifiable
// operations, which throw.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/oprf_nistp.hpp"

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

struct Vectors {  // RFC 9497 A.3 / A.4: the keys of the three modes, the first vector of modes 0 and 1
    const char *sk0, *sk1, *pk1, *pk2, *blind, *blinded0, *evaluated0, *output0, *output1, *dst0;
};

template <class C>
static int run(const Vectors &v) {
    const Bytes seed(32, 0xa3), info = hex("74657374206b6579");
    const oprf::PrivateKey k0 = nistp::DeriveKey<C>(oprf::BaseMode, seed, info), k1 = nistp::DeriveKey<C>(oprf::VerifiableMode, seed, info),
                           k2 = nistp::DeriveKey<C>(oprf::PartialObliviousMode, seed, info);
    CHECK(k0.MarshalBinary() == hex(v.sk0));
    CHECK(k1.MarshalBinary() == hex(v.sk1));
    CHECK(k1.Public().MarshalBinary() == hex(v.pk1));
    CHECK(k2.Public().MarshalBinary() == hex(v.pk2));

    const size_t n = 65;
    List inputs, blinds;
    for (size_t i = 0; i < n; i++) {
        inputs.push_back(i == 0 ? hex("00") : pattern((i * 5) % 90, 100 + i));
        Bytes b = pattern(C::Ns, 300 + i);  // the top byte cleared, the low bit set: below the group order, not zero
        b[0] = 0;
        b[C::Ns - 1] |= 1;
        blinds.push_back(i == 0 ? hex(v.blind) : b);
    }
    const nistp::Client<C> client(oprf::BaseMode);
    const nistp::Server<C> server(k0);
    auto b = client.DeterministicBlind(inputs, blinds);
    CHECK(b.second.Elements.size() == n);
    CHECK(b.second.Elements[0] == hex(v.blinded0));
    const oprf::Evaluation ev = server.Evaluate(b.second);
    CHECK(ev.Elements[0] == hex(v.evaluated0));
    const List out = client.Finalize(b.first, ev), full = server.FullEvaluate(inputs);
    CHECK(out[0] == hex(v.output0));
    CHECK(out.size() == n && out == full);
    for (size_t i = 1; i < n; i++) CHECK(out[i].size() == C::Nh && out[i] != out[0]);

    const nistp::VerifiableServer<C> vserver(k1);
    CHECK(vserver.FullEvaluate({hex("00")})[0] == hex(v.output1));
    CHECK(throws<oprf::ErrModeNotServed>([&] { nistp::Client<C>(oprf::VerifiableMode).Finalize(b.first, ev); }));
    CHECK(throws<oprf::ErrModeNotServed>([&] { vserver.Evaluate(b.second, blinds[1]); }));

    // the group level: a public key is sk G, k^-1 (k P) = P, one scalar for the batch, the hashes answer per item
    using G = nistp::Group<C>;
    CHECK(G::MulGen({k1.MarshalBinary()}).first[0] == k1.Public().MarshalBinary());
    auto unblinded = G::MulInverse(blinds, b.second.Elements);
    const Bytes dst = hex(v.dst0);  // "HashToGroup-" || the mode-0 context
    CHECK(unblinded.first == G::HashToElement(inputs, dst));
    auto shared = G::Mul({k0.MarshalBinary()}, b.second.Elements);
    CHECK(shared.first == ev.Elements);
    const List scalars = G::HashToScalar(inputs, dst), nu = G::HashToElementNonUniform(inputs, dst);
    CHECK(scalars.size() == n && scalars[1] != scalars[2] && scalars[1].size() == C::Ns);
    CHECK(nu.size() == n && nu[1].size() == C::Ne && nu[1] != unblinded.first[1] && (nu[1][0] == 2 || nu[1][0] == 3));
    auto zero_times = G::Mul({Bytes(C::Ns, 0)}, {ev.Elements[3]});  // the identity: a zero row, ok = 1
    CHECK(zero_times.second[0] == 1 && zero_times.first[0] == Bytes(C::Ne, 0));

    // what the protocol refuses
    List bad_blinds = blinds;
    bad_blinds[33] = Bytes(C::Ns, 0);
    CHECK(throws<oprf::ErrInvalidScalar>([&] { client.DeterministicBlind(inputs, bad_blinds); }));
    bad_blinds[33] = Bytes(C::Ns, 0xff);  // above the order
    CHECK(throws<oprf::ErrInvalidScalar>([&] { client.DeterministicBlind(inputs, bad_blinds); }));
    oprf::EvaluationRequest bad_req = b.second;
    bad_req.Elements[64][0] = 4;  // the uncompressed form's prefix
    CHECK(throws<oprf::ErrInvalidElement>([&] { server.Evaluate(bad_req); }));
    bad_req.Elements[64] = Bytes(C::Ne, 0xff);  // x >= p
    bad_req.Elements[64][0] = 2;
    CHECK(throws<oprf::ErrInvalidElement>([&] { server.Evaluate(bad_req); }));
    oprf::Evaluation bad_ev = ev;
    bad_ev.Elements[1] = Bytes(C::Ne, 0);  // the identity
    CHECK(throws<oprf::ErrInvalidElement>([&] { client.Finalize(b.first, bad_ev); }));
    List long_inputs = {Bytes(65536, 7)};
    CHECK(throws<oprf::ErrInvalidInput>([&] { client.DeterministicBlind(long_inputs, {blinds[0]}); }));
    CHECK(throws<oprf::ErrInvalidInput>([&] { server.FullEvaluate(long_inputs); }));
    return 0;
}

int main() {
    const Vectors p256 = {"159749d750713afe245d2d39ccfaae8381c53ce92d098a9375ee70739c7ac0bf",
                          "ca5d94c8807817669a51b196c34c1b7f8442fde4334a7121ae4736364312fca6",
                          "03e17e70604bcabe198882c0a1f27a92441e774224ed9c702e51dd17038b102462",
                          "030d7ff077fddeec965db14b794f0cc1ba9019b04a2f4fcc1fa525dedf72e2a3e3",
                          "3338fa65ec36e0290022b48eb562889d89dbfa691d1cde91517fa222ed7ad364",
                          "03723a1e5c09b8b9c18d1dcbca29e8007e95f14f4732d9346d490ffc195110368d",
                          "030de02ffec47a1fd53efcdd1c6faf5bdc270912b8749e783c7ca75bb412958832",
                          "a0b34de5fa4c5b6da07e72af73cc507cceeb48981b97b7285fc375345fe495dd",
                          "0412e8f78b02c415ab3a288e228978376f99927767ff37c5718d420010a645a1",
                          "48617368546f47726f75702d4f50524656312d002d503235362d534841323536"};
    const Vectors p384 = {"dfe7ddc41a4646901184f2b432616c8ba6d452f9bcd0c4f75a5150ef2b2ed02ef40b8b92f60ae591bcabd72a6518f188",
                          "051646b9e6e7a71ae27c1e1d0b87b4381db6d3595eeeb1adb41579adbf992f4278f9016eafc944edaa2b43183581779d",
                          "031d689686c611991b55f1a1d8f4305ccd6cb719446f660a30db61b7aa87b46acf59b7c0d4a9077b3da21c25dd482229a0",
                          "02f00f0f1de81e5d6cf18140d4926ffdc9b1898c48dc49657ae36eb1e45deb8b951aaf1f10c82d2eaa6d02aafa3f10d2b6",
                          "504650f53df8f16f6861633388936ea23338fa65ec36e0290022b48eb562889d89dbfa691d1cde91517fa222ed7ad364",
                          "02a36bc90e6db34096346eaf8b7bc40ee1113582155ad3797003ce614c835a874343701d3f2debbd80d97cbe45de6e5f1f",
                          "03af2a4fc94770d7a7bf3187ca9cc4faf3732049eded2442ee50fbddda58b70ae2999366f72498cdbc43e6f2fc184afe30",
                          "ed84ad3f31a552f0456e58935fcc0a3039db42e7f356dcb32aa6d487b6b815a07d5813641fb1398c03ddab5763874357",
                          "3333230886b562ffb8329a8be08fea8025755372817ec969d114d1203d026b4a622beab60220bf19078bca35a529b35c",
                          "48617368546f47726f75702d4f50524656312d002d503338342d534841333834"};
    if (run<nistp::P256>(p256) || run<nistp::P384>(p384)) return 1;
    puts("OK");
    return 0;
}
