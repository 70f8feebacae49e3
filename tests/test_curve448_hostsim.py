"""CPU-side checks of the Curve448 device source: fp448_dev.h, x448_dev.h and ed448_dev.h compiled for the host
(tests/hostsim/curve448_hostsim.hip) against Python integers, hashlib and the checker of tests/curve448.py."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import curve448 as ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = ref.P, ref.L
CARRIED = (1 << 28) + (1 << 9) - 1   # fp448_dev.h: limbs of a carried value are below 2^28 + 2^9
SUM2 = 2 * CARRIED                   # a sum of two carried values
SUM4 = 4 * CARRIED


@pytest.fixture(scope="module")
def hs():
    out = os.path.join(ROOT, "build", "libcurve448_hostsim.so")
    src = os.path.join(ROOT, "tests", "hostsim", "curve448_hostsim.hip")
    hdrs = [os.path.join(ROOT, "circl_amd", "csrc", h) for h in ("fp448_dev.h", "x448_dev.h", "ed448_dev.h", "ed448_base_table.h", "keccak_dev.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "circl_amd", "csrc"), src, "-o", out])
    L_ = C.CDLL(out)
    for f in ("hs_sc_is_canonical", "hs_decode", "hs_double_scalar", "hs_fe_sqrt_ratio", "hs_x448", "hs_bytes_word"):
        getattr(L_, f).restype = C.c_uint32
    L_.hs_fe_mul_small.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L_.hs_bytes_word.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L_.hs_shake.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64]
    L_.hs_double_scalar.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L_.hs_ge_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return L_


def _w(v, nwords):
    return np.array([(v >> (32 * i)) & 0xffffffff for i in range(nwords)], np.uint32)


def _int(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _limbs(v):
    return np.array([(v >> (28 * i)) & 0xfffffff for i in range(16)], np.uint32)


def _val(l):
    return sum(int(x) << (28 * i) for i, x in enumerate(l))


def _full(bound):
    return np.full(16, bound, np.uint32)


def _enc15(b: bytes):
    return np.frombuffer(b + b"\0" * 3, np.uint32).copy()


def _rand_fe(rng, bound):
    return np.array([int(rng.integers(0, bound + 1)) for _ in range(16)], np.uint32)


# ---- the field --------------------------------------------------------------------------------------------------------------
def test_field_products_at_the_documented_bounds(hs):
    rng = np.random.default_rng(1)
    out = np.zeros(16, np.uint32)
    pairs = [(_full(SUM2), _full(SUM2)), (_full(SUM4), _full(CARRIED)), (_full(CARRIED), _full(SUM4)), (_full(CARRIED), _full(CARRIED))]
    pairs += [(_rand_fe(rng, SUM2), _rand_fe(rng, SUM2)) for _ in range(300)]
    pairs += [(_limbs(int.from_bytes(rng.bytes(56), "little")), _limbs(int.from_bytes(rng.bytes(56), "little"))) for _ in range(300)]
    for a, b in pairs:
        hs.hs_fe_mul(_p(out), _p(a), _p(b))
        assert _val(out) % P == _val(a) * _val(b) % P
        assert out.max() <= CARRIED
    for a in [_full(SUM2), _full(CARRIED)] + [_rand_fe(rng, SUM2) for _ in range(300)]:
        hs.hs_fe_sqr(_p(out), _p(a))
        assert _val(out) % P == _val(a) ** 2 % P
        assert out.max() <= CARRIED


def test_field_sub_small_and_carry_at_bounds(hs):
    rng = np.random.default_rng(2)
    out = np.zeros(16, np.uint32)
    big = _full((1 << 31) - 1)  # the largest minuend fe_sub documents
    for a, b in [(big, _full(CARRIED)), (_full(0), _full(CARRIED)), (_full(SUM2), _full(CARRIED)), (_full(0), _full(0))] + [
            (_rand_fe(rng, SUM4), _rand_fe(rng, CARRIED)) for _ in range(300)]:
        hs.hs_fe_sub(_p(out), _p(a), _p(b))
        assert _val(out) % P == (_val(a) - _val(b)) % P
        assert out.max() < (1 << 28) + (1 << 5)
    for a in [_full(0xffffffff), _full(SUM4)] + [_rand_fe(rng, 0xffffffff) for _ in range(100)]:
        for c in (39081, 156326, 2, (1 << 20) - 1):
            hs.hs_fe_mul_small(_p(out), _p(a), c)
            assert _val(out) % P == _val(a) * c % P
            assert out.max() <= CARRIED
        hs.hs_fe_carry(_p(out), _p(a))
        assert _val(out) % P == _val(a) % P and out.max() <= CARRIED


def test_canonical_reduction_and_words(hs):
    rng = np.random.default_rng(3)
    w, l = np.zeros(14, np.uint32), np.zeros(16, np.uint32)
    for v in [0, 1, P - 1, P, P + 1, 2**448 - 1, 2**224, 2**224 - 1] + [int.from_bytes(rng.bytes(56), "little") for _ in range(200)]:
        hs.hs_fe_from_words(_p(l), _p(_w(v, 14)))
        assert _val(l) == v and l.max() < (1 << 28)
        hs.hs_fe_to_words(_p(w), _p(l))
        assert _int(w) == v % P, hex(v)
    for a in [_full(CARRIED), _full((1 << 31) - 1), _full((1 << 28) - 1)] + [_rand_fe(rng, (1 << 31) - 1) for _ in range(200)]:
        hs.hs_fe_to_words(_p(w), _p(a))
        assert _int(w) == _val(a) % P
    # values that are p, p + 1, 2p - 1 ... in non-canonical limb forms
    for v in (P, P + 1, 2 * P - 1, 2 * P, 2 * P + 5, 3 * P - 1):
        a = _limbs(v % (1 << 448))
        a[15] += (v >> 448) << 28
        hs.hs_fe_to_words(_p(w), _p(a))
        assert _int(w) == v % P


def test_inversion_and_sqrt_ratio(hs):
    rng = np.random.default_rng(4)
    w = np.zeros(14, np.uint32)
    for v in [0, 1, 2, P - 1] + [int.from_bytes(rng.bytes(56), "little") % P for _ in range(20)]:
        hs.hs_fe_inv(_p(w), _p(_limbs(v)))
        assert _int(w) == pow(v, P - 2, P)
    squares = nonsquares = 0
    for _ in range(40):
        u, v = (int.from_bytes(rng.bytes(56), "little") % P for _ in range(2))
        ok = hs.hs_fe_sqrt_ratio(_p(w), _p(_limbs(u)), _p(_limbs(v)))
        want = pow(u * pow(v, P - 2, P) % P, (P - 1) // 2, P) == 1
        assert bool(ok) == want
        if want:
            squares += 1
            assert v * _int(w) ** 2 % P == u
        else:
            nonsquares += 1
    assert squares > 5 and nonsquares > 5
    x = 1234567
    assert hs.hs_fe_sqrt_ratio(_p(w), _p(_limbs(x * x * 7 % P)), _p(_limbs(7))) == 1 and _int(w) in (x, P - x)
    assert hs.hs_fe_sqrt_ratio(_p(w), _p(_limbs(0)), _p(_limbs(5))) == 1 and _int(w) == 0


# ---- X448 -------------------------------------------------------------------------------------------------------------------
def test_x448_ladder(hs):
    g = load_golden("curve448.json.gz")
    out = np.zeros(14, np.uint32)
    for v in g["x448_kat"]:
        k, u = (np.frombuffer(bytes.fromhex(v[f]), np.uint32).copy() for f in ("scalar", "input"))
        assert hs.hs_x448(_p(out), _p(k), _p(u)) == 1
        assert out.tobytes() == bytes.fromhex(v["output"])
    rng = np.random.default_rng(5)
    for _ in range(3):
        k = rng.bytes(56)
        hs.hs_x448(_p(out), _p(np.frombuffer(k, np.uint32).copy()), None)
        assert out.tobytes() == ref.x448(k)[0]
    k = rng.bytes(56)
    for u, ok in [(0, 0), (1, 0), (P - 1, 0), (P, 0), (P + 1, 0), (2**448 - 1, 1), (P - 2, 1), (2, 1)]:
        ub = u.to_bytes(56, "little")
        assert hs.hs_x448(_p(out), _p(np.frombuffer(k, np.uint32).copy()), _p(np.frombuffer(ub, np.uint32).copy())) == ok, hex(u)
        assert out.tobytes() == ref.x448(k, ub)[0]
        if not ok:
            assert out.tobytes() == bytes(56)


# ---- scalars ----------------------------------------------------------------------------------------------------------------
def test_scalar_arithmetic(hs):
    rng = np.random.default_rng(6)
    top = 2**912
    vals = [0, L - 1, L, L + 1, top - 1, (top // L) * L, (top // L) * L - 1, (top // L) * L - L + 1, (top // L - 1) * L, 2**446, 2**448 - 1, 2**896]
    vals += [int.from_bytes(rng.bytes(114), "little") for _ in range(2000)]
    out = np.zeros(14, np.uint32)
    for x in vals:
        hs.hs_sc_reduce(_p(out), _p(_w(x, 29)))
        assert _int(out) == x % L, hex(x)
    for x in [0, L - 1, L, L + 1, 2**448 - 1, 2**447, 3 * L, 4 * L - 1] + [int.from_bytes(rng.bytes(56), "little") for _ in range(500)]:
        if x >= 2**448:
            continue
        hs.hs_sc_reduce_small(_p(out), _p(_w(x, 14)))
        assert _int(out) == x % L, hex(x)
    for a, b, c in [(2**448 - 1,) * 3, (L - 1, 2**448 - 1, L - 1), (0, 0, 0)] + [tuple(int.from_bytes(rng.bytes(56), "little") for _ in range(3)) for _ in range(1000)]:
        hs.hs_sc_muladd(_p(out), _p(_w(a, 14)), _p(_w(b, 14)), _p(_w(c, 14)))
        assert _int(out) == (a * b + c) % L
    inv4 = pow(4, L - 2, L)
    for x in [0, 1, 2, 3, 4, L - 1, L - 2, L - 3, L - 4] + [int.from_bytes(rng.bytes(56), "little") % L for _ in range(500)]:
        hs.hs_sc_div4(_p(out), _p(_w(x, 14)))
        assert _int(out) == x * inv4 % L
    for s, b56, want in [(0, 0, 1), (L - 1, 0, 1), (L, 0, 0), (L + 1, 0, 0), (2**448 - 1, 0, 0), (2**445, 0, 1), (5, 1, 0), (L - 1, 0x80, 0), (0, 0xff, 0)]:
        sw = np.concatenate([_w(s, 14), np.array([b56], np.uint32)])
        assert hs.hs_sc_is_canonical(_p(sw)) == want, (hex(s), b56)


# ---- bytes and SHAKE256 -----------------------------------------------------------------------------------------------------
def test_bytes_word_any_alignment(hs):
    rng = np.random.default_rng(7)
    buf = rng.integers(1, 256, 512, dtype=np.uint8)
    for off in range(8, 16):
        for n in (0, 1, 2, 3, 4, 5, 57, 114):
            row = buf[off:off + n].tobytes()
            for q in range(-6, n + 6):
                want = int.from_bytes(bytes(row[q + i] if 0 <= q + i < n else 0 for i in range(4)), "little")
                assert hs.hs_bytes_word(C.c_void_p(buf.ctypes.data + off), n, q) == want, (off, n, q)


def _shake(hs, dom, ctx, mid, msg, buf, off_c, off_m):
    """the device absorb with ctx and msg placed at the given byte offsets of a scratch buffer"""
    buf[off_c:off_c + len(ctx)] = np.frombuffer(ctx, np.uint8)
    buf[off_m:off_m + len(msg)] = np.frombuffer(msg, np.uint8)
    nw = 15 if len(mid) <= 57 else 29
    mw = np.frombuffer(mid + b"\0" * (4 * nw - len(mid)), np.uint32).copy()
    out = np.zeros(29, np.uint32)
    hs.hs_shake(_p(out), dom, C.c_void_p(buf.ctypes.data + off_c), len(ctx), _p(mw), nw, len(mid), C.c_void_p(buf.ctypes.data + off_m), len(msg))
    return out.tobytes()[:114]


def test_shake256_block_boundaries_and_alignment(hs):
    rng = np.random.default_rng(8)
    buf = np.zeros(4096, np.uint8)
    cases = 0
    for clen in (0, 1, 2, 3, 7, 255):
        for mid_len in (57, 114):
            head = 10 + clen + mid_len
            lens = {0, 1, 2, 3, 4, 5, 63, 64, 300, 1100}
            for blocks in (1, 2, 3, 4):  # the stream ends one before, on and one after a 136-byte block boundary
                lens |= {blocks * 136 - head + d for d in (-1, 0, 1) if blocks * 136 - head + d >= 0}
            for mlen in sorted(lens):
                ctx, mid, msg = rng.bytes(clen), rng.bytes(mid_len), rng.bytes(mlen)
                off_c, off_m = 16 + cases % 4, 512 + (cases // 4) % 4
                want = hashlib.shake_256(ref.dom4(ctx) + mid + msg).digest(114)
                assert _shake(hs, 1, ctx, mid, msg, buf, off_c, off_m) == want, (clen, mid_len, mlen)
                cases += 1
    for mlen in (0, 1, 78, 79, 80, 135, 136, 137, 500):  # no dom4: the seed hash and plain streams
        mid, msg = rng.bytes(57), rng.bytes(mlen)
        assert _shake(hs, 0, b"", mid, msg, buf, 16, 513) == hashlib.shake_256(mid + msg).digest(114)
    assert cases > 150


# ---- points -----------------------------------------------------------------------------------------------------------------
def _decode(hs, b: bytes):
    enc = np.zeros(15, np.uint32)
    ok = hs.hs_decode(_p(enc), _p(_enc15(b)))
    return ok, enc.tobytes()[:57]


def test_decode(hs):
    keys = sorted({bytes.fromhex(v["pk"]) for v in load_golden("curve448.json.gz")["wycheproof"]})
    assert len(keys) == 9
    e = lambda y, top=0: y.to_bytes(56, "little") + bytes([top])
    rejects = [e(P), e(P + 1), e(1, 0x80), e(P - 1, 0x80), e(ref.y_without_x()), e(2**448 - 1)] + [keys[0][:56] + bytes([keys[0][56] | (1 << b)]) for b in range(7)]
    accepts = [e(1), e(P - 1), e(0), e(0, 0x80), ref.encode(ref.T4), ref.encode(ref.neg(ref.T4))]
    rng = np.random.default_rng(9)
    rand = [rng.bytes(56) + bytes([int(rng.integers(0, 2)) << 7]) for _ in range(40)]
    bad = 0
    for b in keys + rejects + accepts + rand:
        pt = ref.decode(b)
        ok, enc = _decode(hs, b)
        assert ok == (pt is not None), b.hex()
        if pt is not None:
            assert enc == ref.encode(pt) == b, b.hex()
        else:
            bad += 1
    assert all(ref.decode(b) is None for b in rejects) and all(ref.decode(b) is not None for b in accepts)
    assert bad >= len(rejects) + 5


def test_fixed_base(hs):
    rng = np.random.default_rng(10)
    out = np.zeros(15, np.uint32)
    scalars = [0, 1, 2, 7, 8, 9, 15, 16, 2**56 - 1, 2**56, L - 1, L, 2**446 - 1, int("7" * 111, 16), int("8" * 111, 16)]
    scalars += [int.from_bytes(rng.bytes(56), "little") >> 2 for _ in range(12)]
    for k in scalars:
        hs.hs_base(_p(out), _p(_w(k, 14)))
        assert out.tobytes()[:57] == ref.base_mult(k), hex(k)


def test_joint_multiplication_and_the_verification_rule(hs):
    rng = np.random.default_rng(11)
    out = np.zeros(15, np.uint32)
    honest = ref.public(bytes(range(57)))
    A0 = ref.decode(honest)
    with_t4, with_t2 = ref.encode(ref.add(A0, ref.T4)), ref.encode(ref.add(A0, ref.T2))
    differs = 0
    for pk in (honest, with_t4, with_t2, ref.encode(ref.IDENTITY), ref.encode(ref.T4)):
        A = ref.decode(pk)
        for s, k in [(0, 0), (1, 0), (0, 1), (L - 1, L - 1), (5, 3)] + [tuple(int.from_bytes(rng.bytes(56), "little") % L for _ in range(2)) for _ in range(2)]:
            assert hs.hs_double_scalar(_p(out), _p(_w(s, 14)), _p(_w(k, 14)), _p(_enc15(pk)), 0) == 1
            plain = ref.encode(ref.add(ref.mul(s, ref.B), ref.mul(k, ref.neg(A))))
            assert out.tobytes()[:57] == plain, (pk.hex(), hex(s), hex(k))
            assert hs.hs_double_scalar(_p(out), _p(_w(s, 14)), _p(_w(k, 14)), _p(_enc15(pk)), 1) == 1
            comb = ref.encode(ref.combined_circl(s, k, ref.neg(A)))
            assert out.tobytes()[:57] == comb, (pk.hex(), hex(s), hex(k))
            # the torsion component of the key drops out of the reference's rule
            if pk in (with_t4, with_t2):
                assert comb == ref.encode(ref.add(ref.mul(s, ref.B), ref.mul(k, ref.neg(A0))))
                differs += comb != plain
    assert differs > 0


def test_point_formulas_at_limb_bounds(hs):
    # every coordinate with every limb at the carried bound, which is what the formulas take from their callers
    c = _full(CARRIED)
    v = _val(c) % P
    X = Y = Z = T = v
    out = np.zeros(64, np.uint32)
    hs.hs_ge_dbl(_p(out), _p(np.concatenate([c] * 4)))
    A, B, Cc = X * X % P, Y * Y % P, 2 * Z * Z % P
    G, E = (A + B) % P, ((X + Y) ** 2 - A - B) % P
    F, H = (G - Cc) % P, (A - B) % P
    assert [_val(out[16 * i:16 * i + 16]) % P for i in range(4)] == [E * F % P, G * H % P, F * G % P, E * H % P]
    assert out.max() <= CARRIED
    for neg in (0, 1):
        hs.hs_ge_add(_p(out), _p(np.concatenate([c] * 4)), _p(np.concatenate([c] * 4)), neg)
        x2, y2, z2, td = (-v) % P if neg else v, v, v, (-v) % P if neg else v
        a, b = X * x2 % P, Y * y2 % P
        e = ((X + Y) * (x2 + y2) - a - b) % P
        w, dz = T * td % P, Z * z2 % P
        f, g, h = (dz + w) % P, (dz - w) % P, (b - a) % P
        assert [_val(out[16 * i:16 * i + 16]) % P for i in range(4)] == [e * f % P, g * h % P, f * g % P, e * h % P], neg
        assert out.max() <= CARRIED
