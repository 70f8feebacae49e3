// tests/ed25519_test.cpp -- the C++ mirror of include/circl/ed25519.hpp on the GPU: sign/schemes_test.go's round trip for
// "Ed25519" and "Ed25519-Dilithium2" (sizes, DeriveKey, Sign / Verify, a flipped bit, ErrContextNotSupported,
// ErrTypeMismatch, wrong lengths) plus the RFC 8032 section 7.1 TEST 1 vector.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/ed25519.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static circl::ed25519::Bytes hex(const char *s) {
    circl::ed25519::Bytes b;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) { unsigned v; sscanf(s + i, "%2x", &v); b.push_back((uint8_t)v); }
    return b;
}

int main() {
    using namespace circl;
    for (const char *name : {"Ed25519", "Ed25519-Dilithium2"}) {
        const ed25519::Scheme &s = ed25519::ByName(name);
        const ed25519::Scheme &other = ed25519::ByName(std::string(name) == "Ed25519" ? "Ed25519-Dilithium2" : "Ed25519");
        CHECK(s.Name() == name && !s.SupportsContext() && s.SeedSize() == 32);
        ed25519::Bytes seed(32);
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 1);
        auto kp = s.DeriveKey(seed);
        CHECK((int)kp.first.packed.size() == s.PublicKeySize() && (int)kp.second.packed.size() == s.PrivateKeySize());
        const ed25519::Bytes msg = {'h', 'e', 'l', 'l', 'o'};
        ed25519::Bytes sig = s.Sign(kp.second, msg);
        CHECK((int)sig.size() == s.SignatureSize());
        CHECK(s.Verify(kp.first, msg, sig));
        CHECK(s.Sign(kp.second, msg) == sig);  // deterministic
        ed25519::Bytes bad = sig;
        bad[bad.size() - 5] ^= 1;
        CHECK(!s.Verify(kp.first, msg, bad));
        CHECK(!s.Verify(kp.first, msg, ed25519::Bytes(sig.begin(), sig.end() - 1)));
        auto pk2 = s.UnmarshalBinaryPublicKey(kp.first.MarshalBinary());
        CHECK(s.Verify(pk2, msg, sig));
        bool threw = false;
        try { sign::SignatureOpts o{"ctx"}; s.Sign(kp.second, msg, &o); } catch (const sign::ErrContextNotSupported &) { threw = true; }
        CHECK(threw);
        threw = false;
        try { s.UnmarshalBinaryPublicKey(ed25519::Bytes(3)); } catch (const sign::ErrPubKeySize &) { threw = true; }
        CHECK(threw);
        threw = false;
        try { other.Verify(kp.first, msg, sig); } catch (const sign::ErrTypeMismatch &) { threw = true; }
        CHECK(threw);
    }
    // RFC 8032 7.1 TEST 1
    const ed25519::Scheme &ed = ed25519::ByName("Ed25519");
    auto kp = ed.DeriveKey(hex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60"));
    CHECK(kp.first.packed == hex("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"));
    CHECK(ed.Sign(kp.second, {}) == hex("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"));
    printf("OK\n");
    return 0;
}
