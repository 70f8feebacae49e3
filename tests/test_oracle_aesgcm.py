"""The checker tests/aesgcm.py on the reference's AES-GCM known answers (tests/golden/aesgcm_hpke.json.gz: the encryptions of the 64
RFC 9180 vectors with aead_id 1 / 2) and, for lengths, against the system libcrypto.  CPU only."""
import ctypes as C
import ctypes.util
import gzip
import json
import os

import numpy as np
import pytest

import aesgcm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aesgcm_hpke.json.gz")
_VECTORS = {}


def vectors(key_bytes):
    """the fixture's encryptions under keys of key_bytes as (key, base_nonce, seq, nonce, aad, pt, ct), read once"""
    if not _VECTORS:
        with gzip.open(GOLDEN, "rt") as f:
            data = json.load(f)
        h = bytes.fromhex
        for d in data:
            _VECTORS.setdefault(len(d["key"]) // 2, []).extend(
                (h(d["key"]), h(d["base_nonce"]), e["seq"], h(e["nonce"]), h(e["aad"]), h(e["pt"]), h(e["ct"])) for e in d["encryptions"])
    return _VECTORS[key_bytes]


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def test_the_fixture_is_what_the_generator_says():
    assert {k: len(vectors(k)) for k in aesgcm.KEY_SIZES} == {16: 192, 32: 192}
    for ks in aesgcm.KEY_SIZES:
        vs = vectors(ks)
        assert {len(v[0]) for v in vs} == {ks} and {v[2] for v in vs} == {0, 1, 2, 4, 255, 256}
        assert {len(v[5]) for v in vs} == {29} and {len(v[4]) for v in vs} <= {7, 8, 9} and all(len(v[6]) == 29 + 16 for v in vs)


@pytest.mark.parametrize("ks", aesgcm.KEY_SIZES)
def test_checker_reproduces_every_encryption(ks):
    for key, base, seq, nonce, aad, pt, ct in vectors(ks):
        assert aesgcm.seq_nonce(base, seq) == nonce                        # base_nonce + seq ...
        assert aesgcm.seal(key, nonce, pt, aad) == ct                      # ... and the explicit nonce
        assert aesgcm.seal(key, aesgcm.seq_nonce(base, seq), pt, aad) == ct
        assert aesgcm.open_(key, nonce, ct, aad) == pt == aesgcm.open_(key, aesgcm.seq_nonce(base, seq), ct, aad)


def test_checker_refuses_what_was_tampered_with():
    for ks in aesgcm.KEY_SIZES:
        key, _, _, nonce, aad, pt, ct = vectors(ks)[3]
        assert aesgcm.open_(key, nonce, flip(ct, 8 * 29 + 77), aad) is None        # the tag
        assert aesgcm.open_(key, nonce, flip(ct, 8 * 28), aad) is None             # the last ciphertext byte
        assert aesgcm.open_(key, nonce, ct, flip(aad, 9)) is None
        assert aesgcm.open_(key, flip(nonce, 50), ct, aad) is None
        assert aesgcm.open_(flip(key, 3), nonce, ct, aad) is None


def test_checker_known_answers():
    """FIPS 197 appendix C.1 / C.3 and test case 4 of the GCM specification (McGrew, Viega)"""
    block = bytes.fromhex("00112233445566778899aabbccddeeff")
    assert aesgcm.encrypt_block(aesgcm.expand_key(bytes(range(16))), block).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert aesgcm.encrypt_block(aesgcm.expand_key(bytes(range(32))), block).hex() == "8ea2b7ca516745bfeafc49904b496089"
    key, iv = bytes.fromhex("feffe9928665731c6d6a8f9467308308"), bytes.fromhex("cafebabefacedbaddecaf888")
    pt = bytes.fromhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a721c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b39")
    aad = bytes.fromhex("feedfacedeadbeeffeedfacedeadbeefabaddad2")
    ct = aesgcm.seal(key, iv, pt, aad)
    assert ct[:8].hex() == "42831ec221777424" and ct[-16:].hex() == "5bc94fbc3221a5db94fae95ae7121a47"


# ---- against the system libcrypto -------------------------------------------------------------------------------------------------
def libcrypto():
    name = ctypes.util.find_library("crypto") or "libcrypto.so.3"
    try:
        L = C.CDLL(name)
        for f in ("EVP_aes_128_gcm", "EVP_aes_256_gcm", "EVP_aes_128_ecb", "EVP_aes_256_ecb", "EVP_CIPHER_CTX_new"):
            getattr(L, f).restype = C.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
    except (OSError, AttributeError):
        pytest.skip("no libcrypto with EVP_aes_128_gcm / EVP_aes_256_gcm on this machine")
    return L


def evp_seal(L, key, nonce, pt, aad):
    EVP_CTRL_AEAD_GET_TAG = 0x10
    cipher = L.EVP_aes_128_gcm() if len(key) == 16 else L.EVP_aes_256_gcm()
    ctx = C.c_void_p(L.EVP_CIPHER_CTX_new())
    try:
        assert L.EVP_EncryptInit_ex(ctx, C.c_void_p(cipher), None, key, nonce) == 1      # (the default IV length of GCM is 12)
        n = C.c_int(0)
        if aad:
            assert L.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
        out = C.create_string_buffer(len(pt) + 16)
        if pt:
            assert L.EVP_EncryptUpdate(ctx, out, C.byref(n), pt, len(pt)) == 1
            assert n.value == len(pt)
        assert L.EVP_EncryptFinal_ex(ctx, None, C.byref(n)) == 1
        tag = C.create_string_buffer(16)
        assert L.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, tag) == 1
        return out.raw[:len(pt)] + tag.raw
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def evp_ecb(L, key, block):
    """one AES block"""
    cipher = L.EVP_aes_128_ecb() if len(key) == 16 else L.EVP_aes_256_ecb()
    ctx = C.c_void_p(L.EVP_CIPHER_CTX_new())
    try:
        assert L.EVP_EncryptInit_ex(ctx, C.c_void_p(cipher), None, key, None) == 1
        assert L.EVP_CIPHER_CTX_set_padding(ctx, 0) == 1
        n, out = C.c_int(0), C.create_string_buffer(32)
        assert L.EVP_EncryptUpdate(ctx, out, C.byref(n), block, 16) == 1 and n.value == 16
        return out.raw[:16]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def test_libcrypto_agrees_with_the_fixture():
    L = libcrypto()
    for ks in aesgcm.KEY_SIZES:
        for key, _, _, nonce, aad, pt, ct in vectors(ks)[::7]:
            assert evp_seal(L, key, nonce, pt, aad) == ct


@pytest.mark.parametrize("ks", aesgcm.KEY_SIZES)
def test_checker_equals_libcrypto_at_every_length(ks):
    """every plaintext length 0 .. 130 x aad length 0 .. 33 (4454 cases per key size) and one plaintext of 4097 bytes: every partial
    final block of text and aad, and the counter's carry out of its low byte"""
    L = libcrypto()
    rng = np.random.default_rng(38 + ks)
    cases = 0
    for pl in range(131):
        for al in range(34):
            key, nonce, pt, aad = rng.bytes(ks), rng.bytes(12), rng.bytes(pl), rng.bytes(al)
            got = aesgcm.seal(key, nonce, pt, aad)
            assert got == evp_seal(L, key, nonce, pt, aad), (pl, al)
            cases += 1
        assert aesgcm.open_(key, nonce, got, aad) == pt
    assert cases == 4454
    key, nonce, pt, aad = rng.bytes(ks), rng.bytes(12), rng.bytes(4097), rng.bytes(13)
    assert aesgcm.seal(key, nonce, pt, aad) == evp_seal(L, key, nonce, pt, aad)
