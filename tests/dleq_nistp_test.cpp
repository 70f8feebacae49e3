// tests/dleq_nistp_test.cpp -- the C++ mirror of the verifiable OPRF modes on P-256 / P-384 (include/circl/oprf_nistp.hpp, namespace
// nistp::proofs) on the GPU, per curve and for modes 1 and 2: DeriveKey -> DeterministicBlind -> Evaluate with its proof -> Finalize on the
// batched RFC 9497 vector of the suite (two inputs; the proof and both outputs are checked against the published values), Finalize equals
// FullEvaluate on a batch of 70, a client that holds another key refuses the proof, a tampered element or proof gives no output, and bad
// randomness throws.  Prints OK on success.
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

struct Vectors {  // RFC 9497 A.3 / A.4, the third (batched) vector of modes 1 and 2
    const char *blind0, *blind1, *r, *proof1, *out1a, *out1b, *proof2, *out2a, *out2b;
};

template <class C>
static List small_blinds(size_t n, unsigned seed) {
    List l;
    for (size_t i = 0; i < n; i++) {
        Bytes b = pattern(C::Ns, seed + i);  // the top byte cleared, the low bit set: below the group order, not zero
        b[0] = 0;
        b[C::Ns - 1] |= 1;
        l.push_back(b);
    }
    return l;
}

template <class C>
static int run(const Vectors &v) {
    namespace pr = nistp::proofs;
    const Bytes seed(32, 0xa3), key_info = hex("74657374206b6579"), info = hex("7465737420696e666f"), r = hex(v.r);
    const oprf::PrivateKey k1 = nistp::DeriveKey<C>(oprf::VerifiableMode, seed, key_info), k2 = nistp::DeriveKey<C>(oprf::PartialObliviousMode, seed, key_info);
    const List inputs = {hex("00"), hex("5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a")}, blinds = {hex(v.blind0), hex(v.blind1)};

    // mode 1 on the published vector
    const pr::VerifiableServer<C> vs(k1);
    const pr::VerifiableClient<C> vc(k1.Public());
    auto b1 = vc.DeterministicBlind(inputs, blinds);
    const oprf::Evaluation e1 = vs.Evaluate(b1.second, r);
    CHECK(e1.Proof == hex(v.proof1));
    const List o1 = vc.Finalize(b1.first, e1);
    CHECK(o1.size() == 2 && o1[0] == hex(v.out1a) && o1[1] == hex(v.out1b));
    CHECK(o1 == vs.FullEvaluate(inputs));

    // mode 2 on the published vector
    const pr::PartialObliviousServer<C> ps(k2);
    const pr::PartialObliviousClient<C> pc(k2.Public());
    auto b2 = pc.DeterministicBlind(inputs, blinds);
    const oprf::Evaluation e2 = ps.Evaluate(b2.second, info, r);
    CHECK(e2.Proof == hex(v.proof2));
    const List o2 = pc.Finalize(b2.first, e2, info);
    CHECK(o2.size() == 2 && o2[0] == hex(v.out2a) && o2[1] == hex(v.out2b));
    CHECK(o2 == ps.FullEvaluate(inputs, info));

    // a batch over one wavefront: Finalize equals FullEvaluate in both modes
    const size_t n = 70;
    List many;
    for (size_t i = 0; i < n; i++) many.push_back(pattern((i * 5) % 90, 100 + i));
    const List mb = small_blinds<C>(n, 300);
    auto m1 = vc.DeterministicBlind(many, mb);
    const oprf::Evaluation me1 = vs.Evaluate(m1.second, r);
    CHECK(me1.Proof.size() == 2 * C::Ns && vc.Finalize(m1.first, me1) == vs.FullEvaluate(many));
    auto m2 = pc.DeterministicBlind(many, mb);
    const oprf::Evaluation me2 = ps.Evaluate(m2.second, info, r);
    CHECK(pc.Finalize(m2.first, me2, info) == ps.FullEvaluate(many, info));

    // what the clients refuse: a proof for another key, another info, a tampered element, a tampered proof
    CHECK(throws<oprf::ErrInvalidProof>([&] { pr::VerifiableClient<C>(k2.Public()).Finalize(m1.first, me1); }));
    CHECK(throws<oprf::ErrInvalidProof>([&] { pr::PartialObliviousClient<C>(k1.Public()).Finalize(m2.first, me2, info); }));
    CHECK(throws<oprf::ErrInvalidProof>([&] { pc.Finalize(m2.first, me2, hex("7465737420696e666e")); }));
    oprf::Evaluation bad = me1;
    bad.Elements[69] = me1.Elements[0];
    CHECK(throws<oprf::ErrInvalidProof>([&] { vc.Finalize(m1.first, bad); }));
    bad = me1;
    bad.Proof[C::Ns + 3] ^= 0x10;
    CHECK(throws<oprf::ErrInvalidProof>([&] { vc.Finalize(m1.first, bad); }));
    bad = me2;
    bad.Proof.pop_back();
    CHECK(throws<oprf::ErrInvalidProof>([&] { pc.Finalize(m2.first, bad, info); }));
    // what the servers refuse: randomness that is zero or not below the order, an element that does not decode
    CHECK(throws<oprf::ErrInvalidScalar>([&] { vs.Evaluate(m1.second, Bytes(C::Ns, 0)); }));
    CHECK(throws<oprf::ErrInvalidScalar>([&] { ps.Evaluate(m2.second, info, Bytes(C::Ns, 0xff)); }));
    oprf::EvaluationRequest bad_req = m1.second;
    bad_req.Elements[64][0] = 4;
    CHECK(throws<oprf::ErrInvalidElement>([&] { vs.Evaluate(bad_req, r); }));
    CHECK(throws<oprf::ErrInvalidInput>([&] { ps.Evaluate(m2.second, Bytes(65536, 1), r); }));
    return 0;
}

int main() {
    const Vectors p256 = {"3338fa65ec36e0290022b48eb562889d89dbfa691d1cde91517fa222ed7ad364", "f9db001266677f62c095021db018cd8cbb55941d4073698ce45c405d1348b7b1",
                          "350e8040f828bf6ceca27405420cdf3d63cb3aef005f40ba51943c8026877963",
                          "bdcc351707d02a72ce49511c7db990566d29d6153ad6f8982fad2b435d6ce4d60da1e6b3fa740811bde34dd4fe0aa1b5fe6600d0440c9ddee95ea7fad7a60cf2",
                          "0412e8f78b02c415ab3a288e228978376f99927767ff37c5718d420010a645a1", "771e10dcd6bcd3664e23b8f2a710cfaaa8357747c4a8cbba03133967b5c24f18",
                          "8fbd85a32c13aba79db4b42e762c00687d6dbf9c8cb97b2a225645ccb00d9d7580b383c885cdfd07df448d55e06f50f6173405eee5506c0ed0851ff718d13e68",
                          "193a92520bd8fd1f37accb918040a57108daa110dc4f659abe212636d245c592", "1e6d164cfd835d88a31401623549bf6b9b306628ef03a7962921d62bc5ffce8c"};
    const Vectors p384 = {"504650f53df8f16f6861633388936ea23338fa65ec36e0290022b48eb562889d89dbfa691d1cde91517fa222ed7ad364",
                          "803d955f0e073a04aa5d92b3fb739f56f9db001266677f62c095021db018cd8cbb55941d4073698ce45c405d1348b7b1",
                          "a097e722ed2427de86966910acba9f5c350e8040f828bf6ceca27405420cdf3d63cb3aef005f40ba51943c8026877963",
                          "6d8dcbd2fc95550a02211fb78afd013933f307d21e7d855b0b1ed0af78076d8137ad8b0a1bfa05676d325249c1dbb9a52bd81b1c2b7b0efc77cf7b278e1c947f6283f1d4c5"
                          "13053fc0ad19e026fb0c30654b53d9cea4b87b037271b5d2e2d0ea",
                          "3333230886b562ffb8329a8be08fea8025755372817ec969d114d1203d026b4a622beab60220bf19078bca35a529b35c",
                          "b91c70ea3d4d62ba922eb8a7d03809a441e1c3c7af915cbc2226f485213e895942cd0f8580e6d99f82221e66c40d274f",
                          "4a0b2fe96d5b2a046a0447fe079b77859ef11a39a3520d6ff7c626aad9b473b724fb0cf188974ec961710a62162a83e97e0baa9eeada73397032d928b3e97b1ea92ad94582"
                          "08302be3681b8ba78bcc17745bac00f84e0fdc98a6a8cba009c080",
                          "0188653cfec38119a6c7dd7948b0f0720460b4310e40824e048bf82a16527303ed449a08caf84272c3bbc972ede797df",
                          "ff2a527a21cc43b251a567382677f078c6e356336aec069dea8ba36995343ca3b33bb5d6cf15be4d31a7e6d75b30d3f5"};
    if (run<nistp::P256>(p256) || run<nistp::P384>(p384)) return 1;
    puts("OK");
    return 0;
}
