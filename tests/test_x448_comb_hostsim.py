"""X448 KeyGen on the Ed448 comb (x448_dev.h base_mult_comb), compiled for the host (tests/hostsim/x448_comb_hostsim.hip), against
the ladder of the same header and the checker of tests/curve448.py -- and the identity it rests on, on Python integers: RFC 7748's
4-isogeny (x, y) -> u = y^2 / x^2 from edwards448 to curve448 is a group homomorphism that sends the Ed448 base point to u = 5."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import curve448 as ref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = ref.P, ref.L


@pytest.fixture(scope="module")
def hs():
    out = os.path.join(ROOT, "build", "libx448_comb_hostsim.so")
    src = os.path.join(ROOT, "tests", "hostsim", "x448_comb_hostsim.hip")
    hdrs = [os.path.join(ROOT, "circl_amd", "csrc", h) for h in ("fp448_dev.h", "x448_dev.h", "ed448_dev.h", "ed448_base_table.h", "keccak_dev.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "circl_amd", "csrc"), src, "-o", out])
    L_ = C.CDLL(out)
    L_.hs_x448_base_comb.argtypes = L_.hs_x448_base_ladder.argtypes = [C.c_void_p, C.c_void_p]
    L_.hs_x448_base_comb.restype = L_.hs_x448_base_ladder.restype = None
    return L_


def _u_of(pt):
    """the image of an Edwards point under RFC 7748's isogeny: u = y^2 / x^2"""
    x, y = ref.affine(pt)
    return y * y * pow(x * x, P - 2, P) % P


def _both(hs, scalar: bytes):
    k = np.frombuffer(scalar, np.uint32).copy()
    comb, ladder = np.zeros(14, np.uint32), np.zeros(14, np.uint32)
    hs.hs_x448_base_comb(comb.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p))
    hs.hs_x448_base_ladder(ladder.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p))
    return comb.tobytes(), ladder.tobytes()


def _check(hs, scalar: bytes):
    comb, ladder = _both(hs, scalar)
    want = ref.x448(scalar)[0]
    assert ladder == want, scalar.hex()
    assert comb == want, scalar.hex()


def test_the_isogeny_sends_the_base_point_to_5_and_commutes_with_scalars():
    assert _u_of(ref.B) == 5
    rng = np.random.default_rng(21)
    inv4 = pow(4, L - 2, L)
    for _ in range(20):
        k = ref.clamp448(rng.bytes(56))
        want = ref.x448_raw(k, 5)
        assert _u_of(ref.mul(k % L, ref.B)) == want
        # ... and with no factor in between: k / 4, k / 2 and 4 k all give another point
        for other in (k * inv4 % L, k * pow(2, L - 2, L) % L, 4 * k % L):
            assert _u_of(ref.mul(other, ref.B)) != want


def test_the_one_clamped_multiple_of_the_order():
    # clamped: a multiple of 4 in [2^447, 2^448).  2 l < 2^447 < 3 l < 4 l < 2^448 < 5 l, 3 l is odd: k = 4 l is the only clamped
    # scalar with [k]B the identity.  The ladder ends at the point at infinity there and gives 0; y^2 / x^2 with 0 inverted to 0 too.
    assert 2 * L < 2**447 < 3 * L < 4 * L < 2**448 < 5 * L and 3 * L % 4
    assert ref.clamp448((4 * L).to_bytes(56, "little")) == 4 * L
    assert ref.x448_raw(4 * L, 5) == 0
    x, y = ref.affine(ref.mul(4 * L % L, ref.B))
    assert (x, y) == (0, 1) and y * y * pow(x * x, P - 2, P) % P == 0


def test_comb_rfc7748_private_keys(hs):
    g = load_golden("curve448.json.gz")
    seen = 0
    for v in g["x448_kat"]:
        _check(hs, bytes.fromhex(v["scalar"]))
        seen += 1
    assert seen >= 2


def test_comb_all_zero_and_all_ones(hs):
    _check(hs, bytes(56))
    _check(hs, b"\xff" * 56)


def test_comb_scalars_around_multiples_of_the_order(hs):
    """clamped values 4 j next to 3 l and 4 l (4 l itself among them: the identity) and the ends of the clamped range: k mod l is
    then just below l or next to 0, where the reduction's masked subtraction and the recoding's top digit are decided"""
    cases = []
    base = (3 * L) // 4 * 4
    cases += [base + 4 * j for j in range(-3, 5)] + [4 * L + 4 * j for j in range(-4, 5)]
    cases += [2**447 + 4 * j for j in range(0, 4)] + [2**448 - 4 * j for j in range(1, 5)]
    lo = hi = 0
    for k in cases:
        assert 2**447 <= k < 2**448 and k % 4 == 0
        r = k % L
        lo += r < 2**64
        hi += r > L - 2**64
        _check(hs, k.to_bytes(56, "little"))  # (clamping leaves it as it is)
    assert lo >= 4 and hi >= 4


def test_comb_random_scalars(hs):
    rng = np.random.default_rng(22)
    for _ in range(200):
        s = rng.bytes(56)
        comb, ladder = _both(hs, s)
        assert comb == ladder, s.hex()
    for _ in range(8):  # (the Python ladder is the slow part: the hostsim ladder above stands in for it, itself checked here)
        _check(hs, rng.bytes(56))
