// tests/hostsim/hpke_hostsim.hip -- TEST INFRASTRUCTURE: runs the lane-local __host__ __device__ functions of
// circl_amd/csrc/sha256_dev.h, hkdf_dev.h and dhkem_kernels.h on the CPU (their host instantiation), so that the CPU-only test
// tier can check the very source the HPKE DHKEM kernels are built from against hashlib and tests/hpke_dhkem.py.  Nothing here is
// linked into libcirclhip.so.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dhkem_kernels.h"

using namespace circl;
using dhkem::X25519;
using dhkem::X448;

namespace {
// the message shapes of the two KEMs: ikm / dh of 1 or 2 rows, kemCtx of 2 or 3 rows
template <class C>
int extract(uint32_t *prk, int label, int rows, const uint32_t *ikm) {
    using H = typename C::H;
    if (label == 0 && rows == 1) hkdf::labeled_extract<H, C::KEM_ID, C::W>(prk, "dkp_prk", ikm);
    else if (label == 1 && rows == 1) hkdf::labeled_extract<H, C::KEM_ID, C::W>(prk, "eae_prk", ikm);
    else if (label == 1 && rows == 2) hkdf::labeled_extract<H, C::KEM_ID, 2 * C::W>(prk, "eae_prk", ikm);
    else return -1;
    return 0;
}
template <class C>
int expand(uint32_t *out, const uint32_t *prk, int label, int rows, const uint32_t *info) {
    using H = typename C::H;
    if (label == 0 && rows == 0) hkdf::labeled_expand<H, C::KEM_ID, 4 * C::W, 0>(out, prk, "sk", info);
    else if (label == 1 && rows == 2) hkdf::labeled_expand<H, C::KEM_ID, H::OUT, 2 * C::W>(out, prk, "shared_secret", info);
    else if (label == 1 && rows == 3) hkdf::labeled_expand<H, C::KEM_ID, H::OUT, 3 * C::W>(out, prk, "shared_secret", info);
    else return -1;
    return 0;
}
}  // namespace

extern "C" {

// SHA-256(head || msg): head_words in {0, 8, 16}
void hs_sha256(uint32_t *out, const uint32_t *head, int head_words, const uint8_t *msg, uint64_t len) {
    if (head_words == 16) sha256::hash<16>(out, head, msg, len);
    else if (head_words == 8) sha256::hash<8>(out, head, msg, len);
    else sha256::hash<0>(out, nullptr, msg, len);
}

// label: 0 = "dkp_prk" / "sk", 1 = "eae_prk" / "shared_secret"; rows: the ikm / info length in key rows
int hs_labeled_extract(int kem, uint32_t *prk, int label, int rows, const uint32_t *ikm) {
    return kem == 0x20 ? extract<X25519>(prk, label, rows, ikm) : kem == 0x21 ? extract<X448>(prk, label, rows, ikm) : -1;
}
int hs_labeled_expand(int kem, uint32_t *out, const uint32_t *prk, int label, int rows, const uint32_t *info) {
    return kem == 0x20 ? expand<X25519>(out, prk, label, rows, info) : kem == 0x21 ? expand<X448>(out, prk, label, rows, info) : -1;
}

#define BOTH(call25519, call448) (kem == 0x20 ? (call25519) : (call448))
void hs_derive_keypair(int kem, const uint32_t *ikm, uint32_t *sk, uint32_t *pk) {
    if (kem == 0x20) dhkem::op_derive_keypair<X25519>(ikm, sk, pk);
    else dhkem::op_derive_keypair<X448>(ikm, sk, pk);
}
uint32_t hs_encap(int kem, const uint32_t *pkR, const uint32_t *ikmE, uint32_t *enc, uint32_t *ss) {
    return BOTH(dhkem::op_encap<X25519>(pkR, ikmE, enc, ss), dhkem::op_encap<X448>(pkR, ikmE, enc, ss));
}
uint32_t hs_decap(int kem, const uint32_t *skR, const uint32_t *pkR, const uint32_t *enc, uint32_t *ss) {
    return BOTH(dhkem::op_decap<X25519>(skR, pkR, enc, ss), dhkem::op_decap<X448>(skR, pkR, enc, ss));
}
uint32_t hs_auth_encap(int kem, const uint32_t *pkR, const uint32_t *skS, const uint32_t *pkS, const uint32_t *ikmE, uint32_t *enc, uint32_t *ss) {
    return BOTH(dhkem::op_auth_encap<X25519>(pkR, skS, pkS, ikmE, enc, ss), dhkem::op_auth_encap<X448>(pkR, skS, pkS, ikmE, enc, ss));
}
uint32_t hs_auth_decap(int kem, const uint32_t *skR, const uint32_t *pkR, const uint32_t *enc, const uint32_t *pkS, uint32_t *ss) {
    return BOTH(dhkem::op_auth_decap<X25519>(skR, pkR, enc, pkS, ss), dhkem::op_auth_decap<X448>(skR, pkR, enc, pkS, ss));
}

}  // extern "C"
