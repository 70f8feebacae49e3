"""CPU-side checks of the HPKE DHKEM device source: sha256_dev.h, hkdf_dev.h and the operations of dhkem_kernels.h compiled for the
host (tests/hostsim/hpke_hostsim.hip) against hashlib and the checker tests/hpke_dhkem.py on the RFC 9180 vectors."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import hpke_dhkem as hp
from conftest import hx, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = load_golden("hpke_dhkem.json.gz")
KEMS = [0x20, 0x21]


def _deps():
    from circl_amd import build
    src = os.path.join(ROOT, "tests", "hostsim", "hpke_hostsim.hip")
    return src, [src] + [os.path.join(build.CSRC, h) for h in os.listdir(build.CSRC) if h.endswith(".h")]


@pytest.fixture(scope="module")
def hs():
    out = os.path.join(ROOT, "build", "libhpke_hostsim.so")
    src, deps = _deps()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "circl_amd", "csrc"), src, "-o", out])
    L = C.CDLL(out)
    for f in ("hs_encap", "hs_decap", "hs_auth_encap", "hs_auth_decap"):
        getattr(L, f).restype = C.c_uint32
    L.hs_sha256.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _w(b):
    return None if b is None else np.frombuffer(b, np.uint32).copy()


def _sha(hs, head, msg, off=0):
    out = np.zeros(8, np.uint32)
    h = _w(head) if head else np.zeros(1, np.uint32)
    buf = np.zeros(len(msg) + 16, np.uint8)   # the device reads the aligned dwords that hold the message
    base = (-buf.ctypes.data) % 4 + off
    buf[base:base + len(msg)] = np.frombuffer(msg, np.uint8)
    hs.hs_sha256(_p(out), _p(h), len(head) // 4, C.c_void_p(buf.ctypes.data + base), len(msg))
    return out.tobytes()


def test_sha256_every_length_and_alignment(hs):
    rng = np.random.default_rng(256)
    for n in range(201):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for off in range(4):
            assert _sha(hs, b"", msg, off) == hashlib.sha256(msg).digest(), (n, off)


def test_sha256_register_heads(hs):
    rng = np.random.default_rng(257)
    for hl in (32, 64):
        head = rng.integers(0, 256, hl, dtype=np.uint8).tobytes()
        for n in range(201):
            msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            assert _sha(hs, head, msg, n % 4) == hashlib.sha256(head + msg).digest(), (hl, n)


@pytest.mark.parametrize("kem", KEMS)
def test_labeled_extract_and_expand_every_shape(hs, kem):
    """51 / 83 and 17 / 92 / 124 bytes for X25519, 75 / 131 and 17 / 140 / 196 for X448"""
    k = hp.Kem(kem)
    rng = np.random.default_rng(kem)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    for label, name, rows in ((0, b"dkp_prk", 1), (1, b"eae_prk", 1), (1, b"eae_prk", 2)):
        ikm = rnd(rows * k.N)
        prk = np.zeros(k.Nh // 4, np.uint32)
        assert hs.hs_labeled_extract(kem, _p(prk), label, rows, _p(_w(ikm))) == 0
        assert prk.tobytes() == k.labeled_extract(b"", name, ikm), (name, rows)
    for label, name, rows, length in ((0, b"sk", 0, k.N), (1, b"shared_secret", 2, k.Nh), (1, b"shared_secret", 3, k.Nh)):
        prk, info = rnd(k.Nh), rnd(rows * k.N)
        out = np.zeros(length // 4, np.uint32)
        assert hs.hs_labeled_expand(kem, _p(out), _p(_w(prk)), label, rows, _p(_w(info)) if rows else None) == 0
        assert out.tobytes() == k.labeled_expand(prk, name, info, length), (name, rows)


class Host:
    """the five operations of dhkem_kernels.h on one item, on the host"""

    def __init__(self, hs, kem):
        self.hs, self.kem, self.k = hs, kem, hp.Kem(kem)

    def _out(self, nbytes):
        return np.full(nbytes // 4, 0xa5a5a5a5, np.uint32)

    def derive_keypair(self, ikm):
        sk, pk = self._out(self.k.N), self._out(self.k.N)
        self.hs.hs_derive_keypair(self.kem, _p(_w(ikm)), _p(sk), _p(pk))
        return sk.tobytes(), pk.tobytes()

    def encap(self, pkR, ikmE):
        enc, ss = self._out(self.k.N), self._out(self.k.Nh)
        ok = self.hs.hs_encap(self.kem, _p(_w(pkR)), _p(_w(ikmE)), _p(enc), _p(ss))
        return enc.tobytes(), ss.tobytes(), ok

    def decap(self, skR, enc, pkR=None):
        ss = self._out(self.k.Nh)
        ok = self.hs.hs_decap(self.kem, _p(_w(skR)), _p(_w(pkR)), _p(_w(enc)), _p(ss))
        return ss.tobytes(), ok

    def auth_encap(self, pkR, skS, ikmE, pkS=None):
        enc, ss = self._out(self.k.N), self._out(self.k.Nh)
        ok = self.hs.hs_auth_encap(self.kem, _p(_w(pkR)), _p(_w(skS)), _p(_w(pkS)), _p(_w(ikmE)), _p(enc), _p(ss))
        return enc.tobytes(), ss.tobytes(), ok

    def auth_decap(self, skR, enc, pkS, pkR=None):
        ss = self._out(self.k.Nh)
        ok = self.hs.hs_auth_decap(self.kem, _p(_w(skR)), _p(_w(pkR)), _p(_w(enc)), _p(_w(pkS)), _p(ss))
        return ss.tobytes(), ok


@pytest.mark.parametrize("kem", KEMS)
def test_operations_on_the_rfc9180_vectors(hs, kem):
    h = Host(hs, kem)
    vs = [v for v in VECTORS if v["kem_id"] == kem]
    assert len(vs) == 32
    for v in vs:
        for who in "ERS":
            if "ikm" + who in v:
                assert h.derive_keypair(hx(v["ikm" + who])) == (hx(v["sk%sm" % who]), hx(v["pk%sm" % who]))
        skR, pkR, enc, ss = hx(v["skRm"]), hx(v["pkRm"]), hx(v["enc"]), hx(v["shared_secret"])
        if v["mode"] in (0, 1):
            assert h.encap(pkR, hx(v["ikmE"])) == (enc, ss, 1)
            assert h.decap(skR, enc) == (ss, 1) and h.decap(skR, enc, pkR) == (ss, 1)
        else:
            skS, pkS = hx(v["skSm"]), hx(v["pkSm"])
            assert h.auth_encap(pkR, skS, hx(v["ikmE"])) == (enc, ss, 1) and h.auth_encap(pkR, skS, hx(v["ikmE"]), pkS) == (enc, ss, 1)
            assert h.auth_decap(skR, enc, pkS) == (ss, 1) and h.auth_decap(skR, enc, pkS, pkR) == (ss, 1)


@pytest.mark.parametrize("kem", KEMS)
def test_low_order_points_give_zero_rows(hs, kem):
    h = Host(hs, kem)
    k = h.k
    sk, pk = k.derive_keypair(bytes(range(k.N)))
    ikm = bytes(range(1, k.N + 1))
    for pt in hp.low_order_points(kem):
        assert h.encap(pt, ikm) == (bytes(k.N), bytes(k.Nh), 0)
        assert h.auth_encap(pt, sk, ikm) == (bytes(k.N), bytes(k.Nh), 0)
        assert h.decap(sk, pt) == (bytes(k.Nh), 0)
        assert h.auth_decap(sk, pk, pt) == (bytes(k.Nh), 0) and h.auth_decap(sk, pt, pk) == (bytes(k.Nh), 0)


def test_bit_255_of_an_x25519_key_enters_kemctx(hs):
    h = Host(hs, 0x20)
    k = h.k
    _, pkR = k.derive_keypair(bytes(32))
    hi = bytearray(pkR)
    hi[31] |= 0x80
    ikm = bytes(range(32))
    enc, ss, ok = h.encap(bytes(hi), ikm)
    assert (enc, ss) == k.encap(bytes(hi), ikm) and ok == 1
    assert enc == h.encap(pkR, ikm)[0] and ss != h.encap(pkR, ikm)[1]
