// tests/ascon_test.cpp -- the C++ mirror include/circl/ascon.hpp on the GPU: the reference's TestAPI case (key and nonce 00..0f,
// "helloworld", Ascon128) and a ragged batch of three per mode through ascon::Cipher.  The expected ciphertexts come from the caller
// (tests/test_gpu_ascon_mirror.py computes them with the checker tests/ascon.py) as hex arguments: argv[1] = the TestAPI
// ciphertext, argv[2 + 3 m + i] = item i of the batch of mode m (Ascon128, Ascon128a, Ascon80pq).
#include <cstdio>
#include <cstring>
#include <string>

#include "circl/ascon.hpp"

using namespace circl;
using ascon::Bytes;
using ascon::List;

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
    if (argc != 11) return fail("usage: ascon_test <hex ct> <9 hex cts>");
    // TestAPI
    Bytes k16(16), nonce(16);
    for (int j = 0; j < 16; j++) k16[j] = nonce[j] = (uint8_t)j;
    const char *hello = "helloworld";
    const Bytes pt(hello, hello + 10);
    ascon::Cipher c(k16, ascon::Ascon128);
    if (c.NonceSize() != 16 || c.Overhead() != 16) return fail("NonceSize / Overhead");
    if (ascon::ModeKeySize(ascon::Ascon128) != 16 || ascon::ModeKeySize(ascon::Ascon128a) != 16 || ascon::ModeKeySize(ascon::Ascon80pq) != 20)
        return fail("ModeKeySize");
    List ct = c.Seal({nonce}, {pt});
    if (ct.size() != 1 || ct[0] != unhex(argv[1])) return fail("TestAPI: Seal");
    List back = c.Open({nonce}, ct);
    if (back.size() != 1 || back[0] != pt || c.LastOpenOk()[0] != 1) return fail("TestAPI: Open");
    ct[0].back() ^= 0xFF;   // TestOpenClearsOnFailure
    back = c.Open({nonce}, ct);
    if (!back[0].empty() || c.LastOpenOk()[0] != 0) return fail("Open accepted a tampered tag");
    // errors
    try {
        ascon::Cipher bad(Bytes(17), ascon::Ascon128);
        return fail("a key of 17 bytes was accepted");
    } catch (const ascon::ErrKeySize &) {
    }
    try {
        ascon::Cipher bad(Bytes(16), (ascon::Mode)3);
        return fail("mode 3 was accepted");
    } catch (const ascon::ErrMode &) {
    }
    try {
        c.Seal({Bytes(15)}, {pt});
        return fail("a nonce of 15 bytes was accepted");
    } catch (const ascon::ErrNonceSize &) {
    }
    try {
        c.Open({nonce}, {Bytes(15)});
        return fail("a ciphertext of 15 bytes was accepted");
    } catch (const ascon::ErrDecryption &) {
    }
    // a ragged batch of three per mode
    const ascon::Mode modes[3] = {ascon::Ascon128, ascon::Ascon128a, ascon::Ascon80pq};
    const size_t pt_len[3] = {0, 9, 40}, aad_len[3] = {5, 0, 17};
    for (int m = 0; m < 3; m++) {
        ascon::Cipher cm(pattern(ascon::ModeKeySize(modes[m]), m, 1), modes[m]);
        List nonces, pts, aads, want;
        for (int i = 0; i < 3; i++) {
            nonces.push_back(pattern(16, i, 2));
            pts.push_back(pattern(pt_len[i], i, 3));
            aads.push_back(pattern(aad_len[i], i, 4));
            want.push_back(unhex(argv[2 + 3 * m + i]));
        }
        if (cm.Seal(nonces, pts, aads) != want) return fail("batch: Seal");
        if (cm.Open(nonces, want, aads) != pts || cm.LastOpenOk() != Bytes(3, 1)) return fail("batch: Open");
        List forged = want;
        forged[1][2] ^= 1;
        const List got = cm.Open(nonces, forged, aads);
        if (got[0] != pts[0] || !got[1].empty() || got[2] != pts[2] || cm.LastOpenOk() != Bytes{1, 0, 1}) return fail("batch: a forged item");
        // no aads at all
        const List plain = cm.Seal(nonces, pts);
        if (cm.Open(nonces, plain) != pts || plain == want) return fail("batch: without aads");
    }
    puts("OK");
    return 0;
}
