// tests/hpke_test.cpp -- the C++ mirror of include/circl/hpke.hpp on the GPU: for both DHKEMs the sizes, RFC 9180 A.1.1 / A.1.3
// (X25519: DeriveKeyPair, base and auth encapsulation against the published enc and shared_secret), round trips, determinism,
// marshalling, the length errors, a low-order point, and a small batch.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/hpke.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class E, class F> static bool throws(F &&f) {
    try { f(); } catch (const E &) { return true; }
    return false;
}

static circl::kem::Bytes hex(const char *s) {
    circl::kem::Bytes b;
    for (; s[0] && s[1]; s += 2) {
        unsigned v;
        sscanf(s, "%2x", &v);
        b.push_back((uint8_t)v);
    }
    return b;
}

static int scheme_checks(const circl::hpke::Scheme &s, int n, int nh) {
    using namespace circl;
    CHECK(s.PublicKeySize() == n && s.PrivateKeySize() == n && s.SeedSize() == n && s.CiphertextSize() == n && s.EncapsulationSeedSize() == n &&
          s.SharedKeySize() == nh);
    kem::Bytes seedR(n), seedS(n), eseed(n);
    for (int i = 0; i < n; i++) seedR[i] = (uint8_t)(5 * i + 3), seedS[i] = (uint8_t)(7 * i + 1), eseed[i] = (uint8_t)(11 * i + 1);
    auto R = s.DeriveKeyPair(seedR), S = s.DeriveKeyPair(seedS);
    CHECK(R.second.Public().Equal(R.first) && s.DeriveKeyPair(seedR).second.Equal(R.second) && !R.first.Equal(S.first));
    auto enc = s.EncapsulateDeterministically(R.first, eseed);
    CHECK((int)enc.first.size() == n && (int)enc.second.size() == nh && s.EncapsulateDeterministically(R.first, eseed) == enc);
    CHECK(s.Decapsulate(R.second, enc.first) == enc.second);
    auto sk2 = s.UnmarshalBinaryPrivateKey(R.second.MarshalBinary());
    CHECK(sk2.Public().Equal(R.first) && s.Decapsulate(sk2, enc.first) == enc.second);
    auto aenc = s.AuthEncapsulateDeterministically(R.first, S.second, eseed);
    CHECK(aenc.first == enc.first && aenc.second != enc.second);
    CHECK(s.AuthDecapsulate(R.second, aenc.first, S.first) == aenc.second);
    CHECK(s.AuthDecapsulate(R.second, aenc.first, R.first) != aenc.second);  // another sender
    CHECK(throws<kem::ErrSeedSize>([&] { s.DeriveKeyPair(kem::Bytes(n - 1)); }));
    CHECK(throws<kem::ErrSeedSize>([&] { s.EncapsulateDeterministically(R.first, kem::Bytes(n + 1)); }));
    CHECK(throws<kem::ErrCiphertextSize>([&] { s.Decapsulate(R.second, kem::Bytes(n - 1)); }));
    CHECK(throws<kem::ErrPubKeySize>([&] { s.UnmarshalBinaryPublicKey(kem::Bytes(n + 1)); }));
    CHECK(throws<kem::ErrPrivKeySize>([&] { s.UnmarshalBinaryPrivateKey(kem::Bytes(n - 1)); }));
    const auto low = s.UnmarshalBinaryPublicKey(kem::Bytes(n, 0));  // u = 0
    CHECK(throws<hpke::ErrInvalidKEMSharedSecret>([&] { s.EncapsulateDeterministically(low, eseed); }));
    CHECK(throws<hpke::ErrInvalidKEMSharedSecret>([&] { s.Decapsulate(R.second, low.packed); }));
    CHECK(throws<hpke::ErrInvalidKEMSharedSecret>([&] { s.AuthDecapsulate(R.second, aenc.first, low); }));
    // a batch of three: item 0 is the single-shot item, item 2 has a low-order pkR
    const size_t m = 3;
    kem::Bytes seeds(n * m), es(n * m), sks(n * m), pks(n * m), cts(n * m), sss(nh * m), sss2(nh * m), ok(m), ok2(m);
    for (size_t i = 0; i < seeds.size(); i++) seeds[i] = i < (size_t)n ? seedR[i] : (uint8_t)(i * 7), es[i] = i < (size_t)n ? eseed[i] : (uint8_t)(i * 13);
    s.DeriveKeyPairBatch(seeds.data(), sks.data(), pks.data(), m);
    CHECK(memcmp(pks.data(), R.first.packed.data(), n) == 0 && memcmp(sks.data(), R.second.packed.data(), n) == 0);
    kem::Bytes pkr = pks;
    memset(pkr.data() + 2 * n, 0, n);
    s.EncapsulateBatch(pkr.data(), es.data(), cts.data(), sss.data(), ok.data(), m);
    CHECK(ok[0] == 1 && ok[1] == 1 && ok[2] == 0 && memcmp(cts.data(), enc.first.data(), n) == 0 && memcmp(sss.data(), enc.second.data(), nh) == 0);
    for (int i = 0; i < n; i++) CHECK(cts[2 * n + i] == 0);
    for (int i = 0; i < nh; i++) CHECK(sss[2 * nh + i] == 0);
    s.DecapsulateBatch(sks.data(), nullptr, cts.data(), sss2.data(), ok2.data(), m, CIRCL_HIP_ALL_DEVICES);
    CHECK(ok2[0] == 1 && ok2[1] == 1 && ok2[2] == 0 && sss == sss2);
    return 0;
}

int main() {
    using namespace circl;
    const hpke::Scheme &x = hpke::KEM_X25519_HKDF_SHA256(), &y = hpke::KEM_X448_HKDF_SHA512();
    CHECK(x.Name() == "HPKE_KEM_X25519_HKDF_SHA256" && y.Name() == "HPKE_KEM_X448_HKDF_SHA512" && x.ID() == 0x20 && y.ID() == 0x21);
    CHECK(throws<kem::ErrDevice>([] { hpke::Scheme bad(0x10); }));
    // RFC 9180 A.1.1 (base) and A.1.3 (auth), DHKEM(X25519, HKDF-SHA256)
    auto R = x.DeriveKeyPair(hex("6db9df30aa07dd42ee5e8181afdb977e538f5e1fec8a06223f33f7013e525037"));
    CHECK(R.second.packed == hex("4612c550263fc8ad58375df3f557aac531d26850903e55a9f23f21d8534e8ac8"));
    CHECK(R.first.packed == hex("3948cfe0ad1ddb695d780e59077195da6c56506b027329794ab02bca80815c4d"));
    auto e = x.EncapsulateDeterministically(R.first, hex("7268600d403fce431561aef583ee1613527cff655c1343f29812e66706df3234"));
    CHECK(e.first == hex("37fda3567bdbd628e88668c3c8d7e97d1d1253b6d4ea6d44c150f741f1bf4431"));
    CHECK(e.second == hex("fe0e18c9f024ce43799ae393c7e8fe8fce9d218875e8227b0187c04e7d2ea1fc"));
    CHECK(x.Decapsulate(R.second, e.first) == e.second);
    auto R3 = x.DeriveKeyPair(hex("f1d4a30a4cef8d6d4e3b016e6fd3799ea057db4f345472ed302a67ce1c20cdec"));
    auto S3 = x.DeriveKeyPair(hex("94b020ce91d73fca4649006c7e7329a67b40c55e9e93cc907d282bbbff386f58"));
    auto a = x.AuthEncapsulateDeterministically(R3.first, S3.second, hex("6e6d8f200ea2fb20c30b003a8b4f433d2f4ed4c2658d5bc8ce2fef718059c9f7"));
    CHECK(a.first == hex("23fb952571a14a25e3d678140cd0e5eb47a0961bb18afcf85896e5453c312e76"));
    CHECK(a.second == hex("2d6db4cf719dc7293fcbf3fa64690708e44e2bebc81f84608677958c0d4448a7"));
    CHECK(x.AuthDecapsulate(R3.second, a.first, S3.first) == a.second);
    CHECK(throws<kem::ErrTypeMismatch>([&] { y.EncapsulateDeterministically(R.first, kem::Bytes(56)); }));
    if (scheme_checks(x, 32, 32) || scheme_checks(y, 56, 64)) return 1;
    printf("OK\n");
    return 0;
}
