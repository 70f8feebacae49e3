// tests/dleq_test.cpp -- the C++ mirror of the verifiable modes (include/circl/oprf.hpp) on the GPU: for modes 1 and 2 the batch of two
// of RFC 9497 A.1 (DeriveKey -> DeterministicBlind -> Evaluate with the proof randomness given as argv[1] / argv[2] and the two blinds as argv[3] / argv[4] -> Finalize, which
// verifies the proof) must equal FullEvaluate; a request of 70 does the same; a swapped element and a flipped proof bit throw
// ErrInvalidProof.  Prints the two proofs and the four outputs in hex (the caller compares them with the published values), then OK.
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

static void print(const char *what, const Bytes &b) {
    printf("%s ", what);
    for (uint8_t x : b) printf("%02x", x);
    printf("\n");
}

static Bytes small_scalar(unsigned seed) {  // 31 pseudo-random bytes: below the group order, not zero
    Bytes b(32);
    for (auto &x : b) x = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    b[0] |= 1;
    b[31] = 0;
    return b;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const Bytes seed(32, 0xa3), key_info = hex("74657374206b6579"), info = hex("7465737420696e666f");
    const List inputs = {hex("00"), hex("5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a")}, blinds = {hex(argv[3]), hex(argv[4])};
    List many_in, many_bl;
    for (unsigned i = 0; i < 70; i++) {
        many_in.push_back(Bytes(i % 11, (uint8_t)i));
        many_bl.push_back(small_scalar(40 + i));
    }

    // mode 1
    {
        const oprf::PrivateKey k = oprf::DeriveKey(oprf::VerifiableMode, seed, key_info);
        const oprf::VerifiableServer server(k);
        const oprf::VerifiableClient client(k.Public());
        auto b = client.DeterministicBlind(inputs, blinds);
        const oprf::Evaluation ev = server.Evaluate(b.second, hex(argv[1]));
        const List out = client.Finalize(b.first, ev);
        CHECK(out == server.FullEvaluate(inputs));
        print("proof1", ev.Proof);
        print("out1", out[0]);
        print("out1", out[1]);
        auto m = client.DeterministicBlind(many_in, many_bl);
        oprf::Evaluation mev = server.Evaluate(m.second, small_scalar(7));
        CHECK(client.Finalize(m.first, mev) == server.FullEvaluate(many_in));
        std::swap(mev.Elements[3], mev.Elements[68]);
        CHECK(throws<oprf::ErrInvalidProof>([&] { client.Finalize(m.first, mev); }));
        oprf::Evaluation bad = ev;
        bad.Proof[40] ^= 1;
        CHECK(throws<oprf::ErrInvalidProof>([&] { client.Finalize(b.first, bad); }));
        CHECK(throws<oprf::ErrInvalidScalar>([&] { server.Evaluate(b.second, Bytes(32, 0)); }));
    }
    // mode 2
    {
        const oprf::PrivateKey k = oprf::DeriveKey(oprf::PartialObliviousMode, seed, key_info);
        const oprf::PartialObliviousServer server(k);
        const oprf::PartialObliviousClient client(k.Public());
        auto b = client.DeterministicBlind(inputs, blinds);
        const oprf::Evaluation ev = server.Evaluate(b.second, info, hex(argv[2]));
        const List out = client.Finalize(b.first, ev, info);
        CHECK(out == server.FullEvaluate(inputs, info));
        print("proof2", ev.Proof);
        print("out2", out[0]);
        print("out2", out[1]);
        auto m = client.DeterministicBlind(many_in, many_bl);
        oprf::Evaluation mev = server.Evaluate(m.second, info, small_scalar(8));
        CHECK(client.Finalize(m.first, mev, info) == server.FullEvaluate(many_in, info));
        CHECK(throws<oprf::ErrInvalidProof>([&] { client.Finalize(m.first, mev, hex("00")); }));  // another info: another tweaked key
        std::swap(mev.Elements[0], mev.Elements[69]);
        CHECK(throws<oprf::ErrInvalidProof>([&] { client.Finalize(m.first, mev, info); }));
    }
    puts("OK");
    return 0;
}
