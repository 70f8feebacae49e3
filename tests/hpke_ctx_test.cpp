// tests/hpke_ctx_test.cpp -- the C++ mirror of the HPKE contexts (include/circl/hpke.hpp: Suite, Sender, Receiver, Sealer, Opener) on the
// GPU: Sender.Setup -> Seal x 3 -> Receiver.Setup -> Open x 3 -> Export on both sides for a batch of 65, with the sequence numbers
// advancing inside the objects; item 0 is the RFC 9180 vector of DHKEM(X25519, HKDF-SHA256), HKDF-SHA256, ChaCha20Poly1305 in base
// mode, whose first three ciphertexts and second export are checked against the published values.  Then the same flow in auth_psk
// mode over X448 / HKDF-SHA512, a forged ciphertext, and an item whose setup fails.  Prints OK on success.
#include <cstdio>
#include <cstring>

#include "circl/hpke.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace circl;
using hpke::List;

template <class E, class F> static bool throws(F &&f) {
    try { f(); } catch (const E &) { return true; }
    return false;
}

static kem::Bytes hex(const char *s) {
    kem::Bytes b;
    for (; s[0] && s[1]; s += 2) {
        unsigned v;
        sscanf(s, "%2x", &v);
        b.push_back((uint8_t)v);
    }
    return b;
}

static kem::Bytes pattern(size_t len, unsigned seed) {
    kem::Bytes b(len);
    for (size_t i = 0; i < len; i++) b[i] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    return b;
}

static int flow(const hpke::Scheme &k, int kdf, bool auth_psk, bool rfc_item0) {
    const size_t n = 65, N = k.PublicKeySize();
    const hpke::Suite suite(k.ID(), kdf, CIRCL_HIP_HPKE_AEAD_CHACHA20POLY1305);
    CHECK(suite.IsValid() && suite.ContextSize() == (kdf == 1 ? 80u : 112u));
    std::vector<hpke::PublicKey> pkR, pkS;
    std::vector<hpke::PrivateKey> skR, skS;
    List seeds, info, psk, psk_id;
    for (size_t i = 0; i < n; i++) {
        auto R = k.DeriveKeyPair(i == 0 && rfc_item0 ? hex("1ac01f181fdf9f352797655161c58b75c656a6cc2716dcb66372da835542e1df") : pattern(N, 100 + i));
        auto S = k.DeriveKeyPair(pattern(N, 300 + i));
        pkR.push_back(R.first), skR.push_back(R.second), pkS.push_back(S.first), skS.push_back(S.second);
        seeds.push_back(i == 0 && rfc_item0 ? hex("909a9b35d3dc4713a5e72a4da274b55d3d3821a37e5d099e74a647db583a904b") : pattern(N, 500 + i));
        info.push_back(i == 0 && rfc_item0 ? hex("4f6465206f6e2061204772656369616e2055726e") : pattern(i, 700 + i));
        psk.push_back(pattern(32 + i % 7, 900 + i)), psk_id.push_back(pattern(1 + i % 5, 1100 + i));
    }
    if (rfc_item0) CHECK(pkR[0].packed == hex("4310ee97d88cc1f088a5576c77ab0cf5c3ac797f3d95139c6c84b5429c59662a"));
    hpke::Sender sender(suite, pkR, info);
    hpke::Receiver receiver(suite, skR, info);
    auto s = auth_psk ? sender.SetupAuthPSK(seeds, skS, psk, psk_id) : sender.Setup(seeds);
    hpke::Sealer &sealer = s.second;
    hpke::Opener opener = auth_psk ? receiver.SetupAuthPSK(s.first, pkS, psk, psk_id) : receiver.Setup(s.first);
    CHECK(sealer.Size() == n && opener.Size() == n);
    for (size_t i = 0; i < n; i++) CHECK(sealer.Ok()[i] == 1 && opener.Ok()[i] == 1 && s.first[i].size() == N);
    if (rfc_item0) CHECK(s.first[0] == hex("1afa08d3dec047a643885163f1180476fa7ddb54c6a8029ea33f95796bf2ac4a"));
    const char *rfc_ct[3] = {"1c5250d8034ec2b784ba2cfd69dbdb8af406cfe3ff938e131f0def8c8b60b4db21993c62ce81883d2dd1b51a28",
                             "6b53c051e4199c518de79594e1c4ab18b96f081549d45ce015be002090bb119e85285337cc95ba5f59992dc98c",
                             "71146bd6795ccc9c49ce25dda112a48f202ad220559502cef1f34271e0cb4b02b4f10ecac6f48c32f878fae86b"};
    List last_ct, last_aad;
    for (int round = 0; round < 3; round++) {
        List pts, aads;
        for (size_t i = 0; i < n; i++) {
            pts.push_back(i == 0 ? hex("4265617574792069732074727574682c20747275746820626561757479") : pattern((i * 3 + round) % 100, 1300 + 3 * i + round));
            aads.push_back(i == 0 ? hex(round == 0 ? "436f756e742d30" : round == 1 ? "436f756e742d31" : "436f756e742d32") : pattern(i % 9, 1500 + i));
        }
        List cts = sealer.Seal(pts, aads);
        for (size_t i = 0; i < n; i++) CHECK(cts[i].size() == pts[i].size() + 16 && sealer.Seq(i) == (uint64_t)round + 1);
        if (rfc_item0) CHECK(cts[0] == hex(rfc_ct[round]));
        if (round == 2) {  // a forged tag on item 64: refused, and the opener's sequence number stays
            List forged = cts;
            forged[64].back() ^= 1;
            List got = opener.Open(forged, aads);
            CHECK(opener.LastOpenOk()[64] == 0 && got[64].empty() && opener.Seq(64) == 2 && opener.Seq(63) == 3 && got[63] == pts[63]);
            List again = opener.Open(cts, aads);  // every other item is now one sequence number ahead
            CHECK(opener.LastOpenOk()[64] == 1 && again[64] == pts[64] && opener.LastOpenOk()[63] == 0 && opener.Seq(63) == 3);
            break;
        }
        List got = opener.Open(cts, aads);
        for (size_t i = 0; i < n; i++) CHECK(opener.LastOpenOk()[i] == 1 && got[i] == pts[i] && opener.Seq(i) == (uint64_t)round + 1);
    }
    List exps;
    for (size_t i = 0; i < n; i++) exps.push_back(i == 0 ? hex("00") : pattern(i % 40, 1700 + i));
    List a = sealer.Export(exps, 32), b = opener.Export(exps, 32);
    CHECK(a == b && a[1].size() == 32 && a[1] != a[2]);
    if (rfc_item0) CHECK(a[0] == hex("8c1df14732580e5501b00f82b10a1647b40713191b7c1240ac80e2b68808ba69"));
    CHECK(sealer.Export({}, 77) == opener.Export({}, 77) && sealer.Export({}, 77)[5].size() == 77);
    return 0;
}

int main() {
    const hpke::Scheme &x = hpke::KEM_X25519_HKDF_SHA256(), &y = hpke::KEM_X448_HKDF_SHA512();
    CHECK(!hpke::Suite(0x10, 1, 3).IsValid() && !hpke::Suite(0x20, 2, 3).IsValid() && !hpke::Suite(0x20, 1, 1).IsValid() && hpke::Suite(0x21, 3, 0xFFFF).IsValid());
    CHECK(throws<hpke::ErrInvalidHPKESuite>([&] { hpke::Sender bad(hpke::Suite(0x20, 1, 2), {}, {}); }));
    if (flow(x, CIRCL_HIP_HPKE_KDF_HKDF_SHA256, false, true)) return 1;
    if (flow(y, CIRCL_HIP_HPKE_KDF_HKDF_SHA512, true, false)) return 1;
    if (flow(x, CIRCL_HIP_HPKE_KDF_HKDF_SHA512, true, false)) return 1;
    // an item whose setup fails is out of use: a low-order recipient key, and an empty psk in a psk mode
    const hpke::Suite suite(0x20, 1, 3);
    auto R = x.DeriveKeyPair(kem::Bytes(32, 7));
    std::vector<hpke::PublicKey> pkR = {R.first, x.UnmarshalBinaryPublicKey(kem::Bytes(32, 0)), R.first};
    hpke::Sender sender(suite, pkR, {});
    auto s = sender.SetupPSK({kem::Bytes(32, 1), kem::Bytes(32, 2), kem::Bytes(32, 3)}, {kem::Bytes(32, 9), kem::Bytes(32, 9), {}}, {{1}, {2}, {3}});
    CHECK(s.second.Ok()[0] == 1 && s.second.Ok()[1] == 0 && s.second.Ok()[2] == 0 && s.first[0].size() == 32 && s.first[1].empty() && s.first[2].empty());
    List cts = s.second.Seal({{1, 2, 3}, {4}, {}});
    CHECK(cts[0].size() == 19 && cts[1].empty() && cts[2].empty() && s.second.Export({}, 8)[1].empty());
    CHECK(throws<hpke::ErrBatchSize>([&] { s.second.Seal({{1}}); }));
    printf("OK\n");
    return 0;
}
