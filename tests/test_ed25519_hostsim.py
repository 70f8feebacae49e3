"""CPU-side checks of the Ed25519 device source: sha512_dev.h and ed25519_dev.h compiled for the host
(tests/hostsim/ed25519_hostsim.hip) against hashlib and the RFC 8032 checker of tests/ed25519.py."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ed25519 as ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = ref.P, ref.L
POS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
BITS = [26, 25] * 5


@pytest.fixture(scope="module")
def hs():
    out = os.path.join(ROOT, "build", "libed25519_hostsim.so")
    src = os.path.join(ROOT, "tests", "hostsim", "ed25519_hostsim.hip")
    hdrs = [os.path.join(ROOT, "circl_amd", "csrc", h) for h in ("sha512_dev.h", "ed25519_dev.h", "x25519_dev.h", "x25519_base_table.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "circl_amd", "csrc"), src, "-o", out])
    L_ = C.CDLL(out)
    for f in ("hs_sc_is_canonical", "hs_decode", "hs_double_scalar"):
        getattr(L_, f).restype = C.c_uint32
    L_.hs_sha512.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    return L_


def _w(v, nwords):
    return np.array([(v >> (32 * i)) & 0xffffffff for i in range(nwords)], np.uint32)


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _words(b: bytes):
    return np.frombuffer(b, np.uint32).copy()


def _sha(hs, head: bytes, msg: bytes):
    out = np.zeros(16, np.uint32)
    h = _words(head) if head else np.zeros(1, np.uint32)
    m = np.frombuffer(msg + b"\0" * 8, np.uint8).copy()  # the device reads the aligned dwords that hold the message
    hs.hs_sha512(_p(out), _p(h), len(head) // 4, _p(m), len(msg))
    return out.tobytes()


def test_sha512_lengths(hs):
    rng = np.random.default_rng(1)
    for n in list(range(301)) + [111, 112, 239, 240, 1000]:
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert _sha(hs, b"", msg) == hashlib.sha512(msg).digest(), n
    for head in (bytes(range(32)), bytes(range(64))):
        for n in (0, 1, 47, 48, 63, 64, 100, 200):
            msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            assert _sha(hs, head, msg) == hashlib.sha512(head + msg).digest(), (len(head), n)


def test_sha512_unaligned_messages(hs):
    rng = np.random.default_rng(2)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8)
    for off in range(8):
        for n in (0, 1, 3, 5, 111, 112, 113, 300):
            out = np.zeros(16, np.uint32)
            hs.hs_sha512(_p(out), None, 0, C.c_void_p(buf.ctypes.data + off), n)
            assert out.tobytes() == hashlib.sha512(buf[off:off + n].tobytes()).digest(), (off, n)


def test_scalar_reduce_and_muladd(hs):
    rng = np.random.default_rng(3)
    vals = [0, L - 1, L, 2 * L, 2**512 - 1, 2**256 - 1, 8 * L - 1] + [int.from_bytes(rng.bytes(64), "little") for _ in range(3000)]
    for x in vals:
        out = np.zeros(8, np.uint32)
        hs.hs_sc_reduce(_p(out), _p(_w(x, 16)))
        assert _int(out) == x % L, hex(x)
    for _ in range(2000):
        a, b, c = (int.from_bytes(rng.bytes(32), "little") for _ in range(3))
        out = np.zeros(8, np.uint32)
        hs.hs_sc_muladd(_p(out), _p(_w(a, 8)), _p(_w(b, 8)), _p(_w(c, 8)))
        assert _int(out) == (a * b + c) % L
    for s, want in [(0, 1), (L - 1, 1), (L, 0), (L + 1, 0), (2**256 - 1, 0), (2**252, 1)]:
        assert hs.hs_sc_is_canonical(_p(_w(s, 8))) == want, hex(s)


def _decode(hs, b: bytes):
    enc = np.zeros(8, np.uint32)
    ok = hs.hs_decode(_p(enc), _p(_words(b)))
    return ok, enc.tobytes()


def test_decode(hs):
    keys = {bytes.fromhex(v["pk"]) for v in load_golden("ed25519.json.gz")["wycheproof"]}
    keys |= {bytes.fromhex(v["pk"]) for v in load_golden("ed25519.json.gz")["rfc8032"][:64]}
    special = [P.to_bytes(32, "little"), (P + 1).to_bytes(32, "little"), (P + 1 | 1 << 255).to_bytes(32, "little"),
               (1 | 1 << 255).to_bytes(32, "little"), (1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little"),
               (P - 1 | 1 << 255).to_bytes(32, "little"), (2**255 - 1).to_bytes(32, "little"), bytes(32), (1 << 255).to_bytes(32, "little")]
    rng = np.random.default_rng(4)
    rand = [rng.bytes(32) for _ in range(200)]
    seen_bad = 0
    for b in sorted(keys) + special + rand:
        pt = ref.decode(b)
        ok, enc = _decode(hs, b)
        assert ok == (pt is not None), b.hex()
        if pt is not None:
            assert enc == ref.encode(pt), b.hex()
        else:
            seen_bad += 1
    assert seen_bad > 50
    # x = 0 with the sign bit set: y = 1 (the identity) and y = p - 1 are rejected, their sign-clear forms accepted
    assert _decode(hs, (1 | 1 << 255).to_bytes(32, "little"))[0] == 0 and _decode(hs, (1).to_bytes(32, "little"))[0] == 1


def test_base_and_double_scalar(hs):
    rng = np.random.default_rng(5)
    scalars = [0, 1, 2, 7, 8, 9, 15, 16, L - 1, L, 2**253 - 1, (2**254) | 8, 2**255 - 8] + [int.from_bytes(rng.bytes(32), "little") >> 1 for _ in range(40)]
    for k in scalars:
        out = np.zeros(8, np.uint32)
        hs.hs_base(_p(out), _p(_w(k, 8)))
        assert out.tobytes() == ref.base_mult(k), hex(k)
    pks = [bytes.fromhex(v["pk"]) for v in load_golden("ed25519.json.gz")["rfc8032"][:12]]
    for j, pk in enumerate(pks):
        for s, k in [(0, 0), (1, 0), (0, 1), (L - 1, L - 1), (2**253 - 1, 2**253 - 1)] + [
                (int.from_bytes(rng.bytes(32), "little") % L, int.from_bytes(rng.bytes(32), "little") % L) for _ in range(3)]:
            out = np.zeros(8, np.uint32)
            assert hs.hs_double_scalar(_p(out), _p(_w(s, 8)), _p(_w(k, 8)), _p(_words(pk))) == 1
            assert out.tobytes() == ref.double_scalar(s, k, pk), (j, hex(s), hex(k))


def _limbs_value(l):
    return sum(int(x) << p for x, p in zip(l, POS))


def test_point_formulas_at_limb_bounds(hs):
    # every limb at the largest value the formulas take from their callers: carried (2^26 + 2^18 / 2^25 + 2^18) for X, Y, Z, T
    # and 2dT; the cached Y+X / 2Z below 2^27.1 (sums of two carried values), Y-X below 2^27.6 (a difference plus 2p)
    carried = np.array([(1 << 26) + (1 << 18) if i % 2 == 0 else (1 << 25) + (1 << 18) for i in range(10)], np.uint32)
    summed = carried * 2
    diff = np.array([int(c) + 2 * ((1 << b) - 1) for c, b in zip(carried, BITS)], np.uint32)
    p = np.concatenate([carried] * 4)
    X, Y, Z, T = (_limbs_value(carried) % P,) * 4
    out = np.zeros(40, np.uint32)
    hs.hs_ge_dbl(_p(out), _p(p))
    A, B = X * X % P, Y * Y % P
    Cc, H = 2 * Z * Z % P, (A + B) % P
    E, G = ((X + Y) ** 2 - H) % P, (B - A) % P
    F = (Cc - G) % P
    want = [E * F % P, G * H % P, F * G % P, E * H % P]
    assert [_limbs_value(out[10 * i:10 * i + 10]) % P for i in range(4)] == want
    assert out.max() < (1 << 27)
    q = np.concatenate([summed, diff, carried, summed])
    for neg in (0, 1):
        hs.hs_ge_add(_p(out), _p(p), _p(q), neg)
        ypx, ymx, t2d, z2 = _limbs_value(summed) % P, _limbs_value(diff) % P, _limbs_value(carried) % P, _limbs_value(summed) % P
        if neg:
            ypx, ymx, t2d = ymx, ypx, (-t2d) % P
        a, b = (Y - X) * ymx % P, (Y + X) * ypx % P
        c, d = T * t2d % P, Z * z2 % P
        e, f, g, h = b - a, d - c, d + c, b + a
        want = [e * f % P, g * h % P, f * g % P, e * h % P]
        assert [_limbs_value(out[10 * i:10 * i + 10]) % P for i in range(4)] == want, neg
