"""The HPKE context checker (tests/hpke_ctx.py) against the RFC 9180 vectors of tests/golden/hpke_ctx.json.gz and, for its
ChaCha20-Poly1305, against the system libcrypto.  CPU only."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import hpke_ctx as hc
from conftest import hx, load_golden

VECTORS = load_golden("hpke_ctx.json.gz")


def test_the_golden_file_holds_the_32_suites():
    keys = sorted((v["kem_id"], v["kdf_id"], v["aead_id"], v["mode"]) for v in VECTORS)
    assert keys == sorted((kem, kdf, aead, mode) for kem in (32, 33) for kdf in (1, 3) for aead in (3, 65535) for mode in range(4))
    assert sum(len(v["encryptions"]) for v in VECTORS) == 96
    for v in VECTORS:
        assert len(hx(v["info"])) == 20
        assert (len(hx(v.get("psk", ""))), len(hx(v.get("psk_id", "")))) == ((32, 22) if v["mode"] in (1, 3) else (0, 0))
        assert [e["seq"] for e in v["encryptions"]] == ([0, 1, 2, 4, 255, 256] if v["aead_id"] == 3 else [])
        for e in v["encryptions"]:
            assert len(hx(e["pt"])) == 29 and 7 <= len(hx(e["aad"])) <= 9
        assert [(x["L"], len(hx(x["exporter_context"]))) for x in v["exports"]] == [(32, 0), (32, 1), (32, 11)]


def test_checker_reproduces_every_vector():
    for v in VECTORS:
        s = hc.Suite(v["kem_id"], v["kdf_id"], v["aead_id"])
        mode, info, psk, psk_id = v["mode"], hx(v["info"]), hx(v.get("psk", "")), hx(v.get("psk_id", ""))
        auth = mode in (2, 3)
        enc, ks = s.setup_sender(mode, hx(v["pkRm"]), hx(v["ikmE"]), info, psk, psk_id, hx(v["skSm"]) if auth else None)
        assert enc == hx(v["enc"])
        assert ks == s.setup_receiver(mode, hx(v["skRm"]), enc, info, psk, psk_id, hx(v["pkSm"]) if auth else None)
        for f in ("key_schedule_context", "secret", "key", "base_nonce", "exporter_secret"):
            assert ks[f] == hx(v[f]), f
        for e in v["encryptions"]:
            assert s.nonce(ks, e["seq"]) == hx(e["nonce"])
            assert s.seal(ks, e["seq"], hx(e["pt"]), hx(e["aad"])) == hx(e["ct"])
            assert s.open(ks, e["seq"], hx(e["ct"]), hx(e["aad"])) == hx(e["pt"])
            assert s.open(ks, e["seq"] + 1, hx(e["ct"]), hx(e["aad"])) is None
        for x in v["exports"]:
            assert s.export(ks, hx(x["exporter_context"]), x["L"]) == hx(x["exported_value"])


def test_psk_inputs_are_verified():
    s = hc.Suite(32, 1, 3)
    for mode, psk, psk_id, good in ((0, b"", b"", True), (0, b"k", b"i", False), (1, b"k", b"i", True), (1, b"", b"i", False), (1, b"k", b"", False),
                                    (2, b"", b"", True), (2, b"k", b"", False), (3, b"k", b"i", True), (3, b"", b"", False)):
        assert (s.key_schedule(mode, bytes(32), b"", psk, psk_id) is not None) == good, (mode, psk, psk_id)


def _libcrypto():
    name = ctypes.util.find_library("crypto") or "libcrypto.so.3"
    try:
        L = C.CDLL(name)
        L.EVP_chacha20_poly1305.restype = C.c_void_p
        L.EVP_CIPHER_CTX_new.restype = C.c_void_p
    except (OSError, AttributeError):
        pytest.skip("no libcrypto with EVP_chacha20_poly1305 on this machine")
    return L


def _evp_seal(L, key, nonce, pt, aad):
    EVP_CTRL_AEAD_GET_TAG = 0x10
    ctx = C.c_void_p(L.EVP_CIPHER_CTX_new())
    try:
        assert L.EVP_EncryptInit_ex(ctx, C.c_void_p(L.EVP_chacha20_poly1305()), None, key, nonce) == 1
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


def test_chacha20poly1305_equals_libcrypto():
    L = _libcrypto()
    rng = np.random.default_rng(8439)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for pl in range(131):
        for al in range(34):
            key, nonce, pt, aad = rnd(32), rnd(12), rnd(pl), rnd(al)
            ct = hc.aead_seal(key, nonce, pt, aad)
            assert ct == _evp_seal(L, key, nonce, pt, aad), (pl, al)
            if (pl + al) % 7 == 0:
                assert hc.aead_open(key, nonce, ct, aad) == pt


def test_poly1305_final_reduction():
    """h reaches 2^130 - 2 >= p before the last subtraction: r = 1, s = 0, 32 bytes of 0xff -> 3"""
    assert hc.poly1305((1).to_bytes(16, "little") + bytes(16), b"\xff" * 32) == (3).to_bytes(16, "little")
