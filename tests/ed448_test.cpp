// tests/ed448_test.cpp -- the C++ mirror of include/circl/ed448.hpp on the GPU: sign/schemes_test.go's round trip for "Ed448" and
// "Ed448-Dilithium3" (sizes, DeriveKey, Sign / Verify, a flipped bit, contexts, ErrContextNotSupported, ErrContextTooLong,
// ErrTypeMismatch, wrong lengths) plus the first two RFC 8032 section 7.4 vectors (blank, and one octet with a context).
// Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/ed448.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static circl::ed448::Bytes hex(const char *s) {
    circl::ed448::Bytes b;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) { unsigned v; sscanf(s + i, "%2x", &v); b.push_back((uint8_t)v); }
    return b;
}

int main() {
    using namespace circl;
    for (const char *name : {"Ed448", "Ed448-Dilithium3"}) {
        const bool plain = std::string(name) == "Ed448";
        const ed448::Scheme &s = ed448::ByName(name);
        const ed448::Scheme &other = ed448::ByName(plain ? "Ed448-Dilithium3" : "Ed448");
        CHECK(s.Name() == name && s.SupportsContext() == plain && s.SeedSize() == 57);
        CHECK(s.PublicKeySize() == (plain ? 57 : 2009) && s.PrivateKeySize() == (plain ? 114 : 4057) && s.SignatureSize() == (plain ? 114 : 3407));
        ed448::Bytes seed(57);
        for (int i = 0; i < 57; i++) seed[i] = (uint8_t)(7 * i + 1);
        auto kp = s.DeriveKey(seed);
        CHECK((int)kp.first.packed.size() == s.PublicKeySize() && (int)kp.second.packed.size() == s.PrivateKeySize());
        const ed448::Bytes msg = {'h', 'e', 'l', 'l', 'o'};
        ed448::Bytes sig = s.Sign(kp.second, msg);
        CHECK((int)sig.size() == s.SignatureSize());
        CHECK(s.Verify(kp.first, msg, sig));
        CHECK(s.Sign(kp.second, msg) == sig);  // deterministic
        ed448::Bytes bad = sig;
        bad[bad.size() - 5] ^= 1;
        CHECK(!s.Verify(kp.first, msg, bad));
        CHECK(!s.Verify(kp.first, msg, ed448::Bytes(sig.begin(), sig.end() - 1)));
        auto pk2 = s.UnmarshalBinaryPublicKey(kp.first.MarshalBinary());
        CHECK(s.Verify(pk2, msg, sig));
        sign::SignatureOpts o{"ctx"}, o2{"cty"}, big{std::string(256, 'x')};
        if (plain) {
            ed448::Bytes csig = s.Sign(kp.second, msg, &o);
            CHECK(csig != sig && s.Verify(kp.first, msg, csig, &o) && !s.Verify(kp.first, msg, csig, &o2) && !s.Verify(kp.first, msg, csig));
            CHECK(!s.Verify(kp.first, msg, csig, &big));
            bool threw = false;
            try { s.Sign(kp.second, msg, &big); } catch (const sign::ErrContextTooLong &) { threw = true; }
            CHECK(threw);
        } else {
            bool threw = false;
            try { s.Sign(kp.second, msg, &o); } catch (const sign::ErrContextNotSupported &) { threw = true; }
            CHECK(threw);
        }
        bool threw = false;
        try { s.UnmarshalBinaryPublicKey(ed448::Bytes(3)); } catch (const sign::ErrPubKeySize &) { threw = true; }
        CHECK(threw);
        threw = false;
        try { other.Verify(kp.first, msg, sig); } catch (const sign::ErrTypeMismatch &) { threw = true; }
        CHECK(threw);
    }
    // RFC 8032 7.4: "Blank", then "1 octet (with context)" (context "foo")
    const ed448::Scheme &ed = ed448::ByName("Ed448");
    auto kp = ed.DeriveKey(hex("6c82a562cb808d10d632be89c8513ebf6c929f34ddfa8c9f63c9960ef6e348a3528c8a3fcc2f044e39a3fc5b94492f8f032e7549a20098f95b"));
    CHECK(kp.first.packed == hex("5fd7449b59b461fd2ce787ec616ad46a1da1342485a70e1f8a0ea75d80e96778edf124769b46c7061bd6783df1e50f6cd1fa1abeafe8256180"));
    CHECK(ed.Sign(kp.second, {}) ==
          hex("533a37f6bbe457251f023c0d88f976ae2dfb504a843e34d2074fd823d41a591f2b233f034f628281f2fd7a22ddd47d7828c59bd0a21bfd3980"
              "ff0d2028d4b18a9df63e006c5d1c2d345b925d8dc00b4104852db99ac5c7cdda8530a113a0f4dbb61149f05a7363268c71d95808ff2e652600"));
    auto kp2 = ed.DeriveKey(hex("c4eab05d357007c632f3dbb48489924d552b08fe0c353a0d4a1f00acda2c463afbea67c5e8d2877c5e3bc397a659949ef8021e954e0a12274e"));
    CHECK(kp2.first.packed == hex("43ba28f430cdff456ae531545f7ecd0ac834a55d9358c0372bfa0c6c6798c0866aea01eb00742802b8438ea4cb82169c235160627b4c3a9480"));
    sign::SignatureOpts foo{"foo"};
    CHECK(ed.Sign(kp2.second, {0x03}, &foo) ==
          hex("d4f8f6131770dd46f40867d6fd5d5055de43541f8c5e35abbcd001b32a89f7d2151f7647f11d8ca2ae279fb842d607217fce6e042f6815ea00"
              "0c85741de5c8da1144a6a1aba7f96de42505d7a7298524fda538fccbbb754f578c1cad10d54d0d5428407e85dcbc98a49155c13764e66c3c00"));
    printf("OK\n");
    return 0;
}
