// tests/aesgcm_test.cpp -- the C++ mirror include/circl/aesgcm.hpp on the GPU: a ragged batch of three per key size through
// aesgcm::Cipher, by explicit nonces and by a base nonce with sequence numbers.  The expected ciphertexts come from the caller
// (tests/test_gpu_aesgcm_mirror.py computes them with the checker tests/aesgcm.py) as hex arguments: argv[1 + 6 k + i] = item i
// under explicit nonces, argv[4 + 6 k + i] = item i under base nonce + sequence number 255 + i, for key size k (16, 32).
#include <cstdio>
#include <cstring>
#include <string>

#include "circl/aesgcm.hpp"

using namespace circl;
using aesgcm::Bytes;
using aesgcm::List;

static Bytes unhex(const char *s) {
    Bytes b;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) b.push_back((uint8_t)std::stoi(std::string(s + i, 2), nullptr, 16));
    return b;
}
// the byte pattern both sides of the test agree on
static Bytes pattern(size_t len, int a, int b) {
    Bytes r(len);
    for (size_t j = 0; j < len; j++) r[j] = (uint8_t)(7 * j + 13 * a + b);
    return r;
}
static int fail(const char *what) {
    printf("FAIL %s\n", what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 13) return fail("usage: aesgcm_test <12 hex cts>");
    // errors
    for (size_t bad : {size_t(0), size_t(15), size_t(24), size_t(33)}) {
        try {
            aesgcm::Cipher c{Bytes(bad)};
            return fail("a key of another size than 16 or 32 bytes was accepted");
        } catch (const aesgcm::ErrKeySize &) {
        }
    }
    const size_t pt_len[3] = {0, 9, 40}, aad_len[3] = {5, 0, 17};
    const int sizes[2] = {aesgcm::KeySize128, aesgcm::KeySize256};
    for (int k = 0; k < 2; k++) {
        aesgcm::Cipher c(pattern(sizes[k], k, 1));
        if (c.NonceSize() != 12 || c.Overhead() != 16) return fail("NonceSize / Overhead");
        List nonces, pts, aads, want, want_seq;
        for (int i = 0; i < 3; i++) {
            nonces.push_back(pattern(12, i, 2));
            pts.push_back(pattern(pt_len[i], i, 3));
            aads.push_back(pattern(aad_len[i], i, 4));
            want.push_back(unhex(argv[1 + 6 * k + i]));
            want_seq.push_back(unhex(argv[4 + 6 * k + i]));
        }
        if (c.Seal(nonces, pts, aads) != want) return fail("batch: Seal");
        if (c.Open(nonces, want, aads) != pts || c.LastOpenOk() != Bytes(3, 1)) return fail("batch: Open");
        List forged = want;
        forged[1][2] ^= 1;
        const List got = c.Open(nonces, forged, aads);
        if (got[0] != pts[0] || !got[1].empty() || got[2] != pts[2] || c.LastOpenOk() != Bytes{1, 0, 1}) return fail("batch: a forged item");
        // no aads at all
        const List plain = c.Seal(nonces, pts);
        if (c.Open(nonces, plain) != pts || plain == want) return fail("batch: without aads");
        // one base nonce, sequence numbers 255, 256, 257
        if (c.SealSeq(nonces[0], 255, pts, aads) != want_seq) return fail("batch: SealSeq");
        if (c.OpenSeq(nonces[0], 255, want_seq, aads) != pts || c.LastOpenOk() != Bytes(3, 1)) return fail("batch: OpenSeq");
        c.OpenSeq(nonces[0], 254, want_seq, aads);
        if (c.LastOpenOk() != Bytes(3, 0)) return fail("batch: OpenSeq under other sequence numbers");
        try {
            c.Seal({Bytes(16)}, {pts[0]});
            return fail("a nonce of 16 bytes was accepted");
        } catch (const aesgcm::ErrNonceSize &) {
        }
        try {
            c.Open({nonces[0]}, {Bytes(15)});
            return fail("a ciphertext of 15 bytes was accepted");
        } catch (const aesgcm::ErrOpen &) {
        }
    }
    puts("OK");
    return 0;
}
