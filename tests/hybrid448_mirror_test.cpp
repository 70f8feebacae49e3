// tests/hybrid448_mirror_test.cpp -- the C++ mirrors of Kyber768-X448 and Kyber1024-X448 (include/circl/hybrid.hpp) against the
// reference's names and sizes (kem/hybrid/hybrid.go:83-93, :123-157) and against the C ABI's own size calls.  Needs no device.
#include <cstdio>
#include <cstring>

#include "circl/hybrid.hpp"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

template <class S>
static int against_abi(int scheme) {
    CHECK((size_t)S::SeedSize == circl_hip_hybrid_seed_size(scheme));
    CHECK((size_t)S::EncapsulationSeedSize == circl_hip_hybrid_eseed_size(scheme));
    CHECK((size_t)S::PublicKeySize == circl_hip_hybrid_pk_size(scheme));
    CHECK((size_t)S::PrivateKeySize == circl_hip_hybrid_sk_size(scheme));
    CHECK((size_t)S::CiphertextSize == circl_hip_hybrid_ct_size(scheme));
    CHECK((size_t)S::SharedKeySize == circl_hip_hybrid_ss_size(scheme));
    // wrong sizes are the reference's errors, before anything reaches the device
    bool threw = false;
    try { S::DeriveKeyPair(typename S::Bytes(S::SeedSize - 1)); } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
    threw = false;
    try { S::EncapsulateDeterministically(typename S::Bytes(S::PublicKeySize), typename S::Bytes(32)); } catch (const typename S::Error &) { threw = true; }
    CHECK(threw);
    threw = false;
    try { S::Decapsulate(typename S::Bytes(S::PrivateKeySize), typename S::Bytes(S::CiphertextSize + 1)); } catch (const typename S::Error &) { threw = true; }
    CHECK(threw);
    return 0;
}

int main() {
    using A = circl::hybrid::Kyber768X448;
    using B = circl::hybrid::Kyber1024X448;
    static_assert(A::PublicKeySize == 1240 && A::PrivateKeySize == 2456 && A::CiphertextSize == 1144 && A::SharedKeySize == 88, "Kyber768-X448");
    static_assert(B::PublicKeySize == 1624 && B::PrivateKeySize == 3224 && B::CiphertextSize == 1624 && B::SharedKeySize == 88, "Kyber1024-X448");
    static_assert(A::SeedSize == 64 && A::EncapsulationSeedSize == 56 && B::SeedSize == 64 && B::EncapsulationSeedSize == 56, "seeds");
    CHECK(!std::strcmp(A::Name(), "Kyber768-X448"));
    CHECK(!std::strcmp(B::Name(), "Kyber1024-X448"));
    if (against_abi<A>(CIRCL_HIP_HYBRID_KYBER768_X448)) return 1;
    if (against_abi<B>(CIRCL_HIP_HYBRID_KYBER1024_X448)) return 1;
    std::printf("hybrid448 mirror ok\n");
    return 0;
}
