// tests/frodo_test.cpp -- the C++ mirror of include/circl/frodo.hpp on the GPU: kem/schemes_test.go's round trip for
// "FrodoKEM-640-SHAKE" (sizes, DeriveKeyPair, EncapsulateDeterministically / Decapsulate, determinism, a flipped bit, marshalling,
// the length errors of frodo.go:517-547) and a small batch.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/frodo.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class E, class F> static bool throws(F &&f) {
    try { f(); } catch (const E &) { return true; }
    return false;
}

int main() {
    using namespace circl;
    const frodo::Scheme &s = frodo::Frodo640Shake();
    CHECK(s.Name() == "FrodoKEM-640-SHAKE");
    CHECK(s.PublicKeySize() == 9616 && s.PrivateKeySize() == 19888 && s.CiphertextSize() == 9720 && s.SharedKeySize() == 16 && s.SeedSize() == 48 &&
          s.EncapsulationSeedSize() == 16);
    kem::Bytes seed(48), eseed(16);
    for (int i = 0; i < 48; i++) seed[i] = (uint8_t)(5 * i + 3);
    for (int i = 0; i < 16; i++) eseed[i] = (uint8_t)(11 * i + 1);
    auto kp = s.DeriveKeyPair(seed);
    CHECK((int)kp.first.packed.size() == s.PublicKeySize() && (int)kp.second.packed.size() == s.PrivateKeySize());
    CHECK(kp.second.Public().Equal(kp.first));
    CHECK(memcmp(kp.second.packed.data(), seed.data(), 16) == 0);  // s leads the private key
    auto kp2 = s.DeriveKeyPair(seed);
    CHECK(kp2.first.Equal(kp.first) && kp2.second.Equal(kp.second));
    auto enc = s.EncapsulateDeterministically(kp.first, eseed);
    CHECK((int)enc.first.size() == s.CiphertextSize() && (int)enc.second.size() == s.SharedKeySize());
    CHECK(s.EncapsulateDeterministically(kp.first, eseed) == enc);
    CHECK(s.Decapsulate(kp.second, enc.first) == enc.second);
    auto sk2 = s.UnmarshalBinaryPrivateKey(kp.second.MarshalBinary());
    auto pk2 = s.UnmarshalBinaryPublicKey(kp.first.MarshalBinary());
    CHECK(s.Decapsulate(sk2, s.EncapsulateDeterministically(pk2, eseed).first) == enc.second);
    kem::Bytes bad = enc.first;
    bad[9719] ^= 1;
    const kem::Bytes rej = s.Decapsulate(kp.second, bad);
    CHECK(rej != enc.second && (int)rej.size() == 16 && s.Decapsulate(kp.second, bad) == rej);
    CHECK(throws<kem::ErrSeedSize>([&] { s.DeriveKeyPair(kem::Bytes(47)); }));
    CHECK(throws<kem::ErrSeedSize>([&] { s.EncapsulateDeterministically(kp.first, kem::Bytes(15)); }));
    CHECK(throws<kem::ErrCiphertextSize>([&] { s.Decapsulate(kp.second, kem::Bytes(9719)); }));
    CHECK(throws<kem::ErrPubKeySize>([&] { s.UnmarshalBinaryPublicKey(kem::Bytes(9615)); }));
    CHECK(throws<kem::ErrPrivKeySize>([&] { s.UnmarshalBinaryPrivateKey(kem::Bytes(19889)); }));
    const frodo::Scheme other;
    CHECK(throws<kem::ErrTypeMismatch>([&] { other.EncapsulateDeterministically(kp.first, eseed); }));
    CHECK(throws<kem::ErrTypeMismatch>([&] { other.Decapsulate(kp.second, enc.first); }));
    // a batch of three: item 0 is the single-shot item
    const size_t n = 3;
    kem::Bytes seeds(48 * n), eseeds(16 * n), pks(9616 * n), sks(19888 * n), cts(9720 * n), sss(16 * n), sss2(16 * n);
    for (size_t i = 0; i < seeds.size(); i++) seeds[i] = i < 48 ? seed[i] : (uint8_t)(i * 7);
    for (size_t i = 0; i < eseeds.size(); i++) eseeds[i] = i < 16 ? eseed[i] : (uint8_t)(i * 13);
    s.DeriveKeyPairBatch(seeds.data(), pks.data(), sks.data(), n);
    s.EncapsulateBatch(pks.data(), eseeds.data(), cts.data(), sss.data(), n);
    s.DecapsulateBatch(sks.data(), cts.data(), sss2.data(), n, CIRCL_HIP_ALL_DEVICES);
    CHECK(sss == sss2);
    CHECK(memcmp(pks.data(), kp.first.packed.data(), 9616) == 0 && memcmp(cts.data(), enc.first.data(), 9720) == 0 && memcmp(sss.data(), enc.second.data(), 16) == 0);
    printf("OK\n");
    return 0;
}
