"""The CPU checker tests/oprf_nistp.py (RFC 9380 / RFC 9497 / SEC 1 restated) against the fixture tests/golden/oprf_nistp.json.gz -- the
reference's 20 hash-to-curve vectors for P-256 / P-384 and the six RFC 9497 entries of suites P256-SHA256 / P384-SHA384 -- and, for the
point arithmetic, against the system libcrypto's EC_POINT_mul.  CPU only."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import oprf_nistp as on
from conftest import hx, load_golden

G = load_golden("oprf_nistp.json.gz")
CURVES = (256, 384)


def entries(curve):
    return [e for e in G["rfc9497"] if e["identifier"] == on.CURVES[curve].name]


def items(v):
    """the (input, blind, blinded, evaluated, output) of every item of a vector (batched ones separate theirs by commas)"""
    cols = [v[k].split(",") for k in ("Input", "Blind", "BlindedElement", "EvaluationElement", "Output")]
    assert len({len(c) for c in cols}) == 1 and len(cols[0]) == v["Batch"]
    return [tuple(hx(x) for x in row) for row in zip(*cols)]


def h2c(curve, kind):
    return G["h2c"]["P%d_%s" % (curve, kind)]


def xy(d):
    return (int(d["x"], 16), int(d["y"], 16))


def test_fixture_shape():
    assert [(e["identifier"], e["mode"]) for e in G["rfc9497"]] == [(on.CURVES[c].name, m) for c in CURVES for m in (0, 1, 2)]
    for c in CURVES:
        assert [len(e["vectors"]) for e in entries(c)] == [2, 3, 3]
        assert [sum(len(items(v)) for v in e["vectors"]) for e in entries(c)] == [2, 4, 4]      # the third of modes 1 and 2 is a batch of two
        for kind in ("RO", "NU"):
            assert [len(v["msg"]) for v in h2c(c, kind)["vectors"]] == [0, 3, 16, 133, 517]


@pytest.mark.parametrize("curve", CURVES)
def test_constants(curve):
    c = on.CURVES[curve]
    f = h2c(curve, "RO")
    assert int(f["field"]["p"], 16) == c.p and int(f["Z"], 16) == c.z and int(f["L"], 16) == c.ell
    assert c.c2 * c.c2 % c.p == -c.z ** 3 % c.p and c.c1 == (c.p - 3) // 4
    assert (c.Ns, c.Ne, c.Nh) == {256: (32, 33, 32), 384: (48, 49, 48)}[curve]


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_curve_vectors(curve):
    c = on.CURVES[curve]
    n = 0
    for kind in ("RO", "NU"):
        f = h2c(curve, kind)
        dst = f["dst"].encode()
        for v in f["vectors"]:
            msg = v["msg"].encode()
            u = c.hash_to_field(msg, dst, 2 if kind == "RO" else 1)
            assert u == [int(x, 16) for x in v["u"]]
            if kind == "RO":
                q0, q1 = c.map_to_curve(u[0]), c.map_to_curve(u[1])
                assert (q0, q1) == (xy(v["Q0"]), xy(v["Q1"]))
                assert c.add(q0, q1) == xy(v["P"])
            else:
                assert c.map_to_curve(u[0]) == xy(v["Q"]) == xy(v["P"])
            assert on.hash_to_group(curve, msg, dst, kind == "NU") == c.encode(xy(v["P"]))
            n += 1
    assert n == 10


@pytest.mark.parametrize("curve", CURVES)
def test_codec(curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(curve)
    for k in list(range(1, 8)) + [c.n - 1, c.n - 2, (c.n + 1) // 2]:
        pt = c.mul(k, c.G)
        assert c.on_curve(pt) and c.decode(c.encode(pt)) == pt
    assert c.encode(None) == bytes(c.Ne) and c.decode(bytes(c.Ne)) is None
    assert c.mul(c.n - 1, c.G) == c.neg(c.G) and c.add(c.G, c.neg(c.G)) is None
    gx = c.G[0].to_bytes(c.Ns, "big")
    for prefix in (0, 4, 5, 1, 255):
        assert c.decode(bytes([prefix]) + gx) is False
    for x in (c.p, c.p + 1, 2 ** (8 * c.Ns) - 1):
        assert c.decode(b"\x02" + x.to_bytes(c.Ns, "big")) is False
    seen = set()
    for _ in range(40):
        b = bytes([2 + int(rng.integers(2))]) + (int.from_bytes(rng.bytes(c.Ns), "big") % c.p).to_bytes(c.Ns, "big")
        pt = c.decode(b)
        seen.add(pt is not False)
        assert pt is False or (c.on_curve(pt) and c.encode(pt) == b)
    assert seen == {True, False}                # about half of all x are on the curve


@pytest.mark.parametrize("curve", CURVES)
def test_fast_multiplication_equals_the_affine_law(curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(7 + curve)
    q = c.mul_affine(12345, c.G)
    for k in list(range(9)) + [c.n - 1, c.n - 2, c.n, c.n + 1, (c.n + 1) // 2] + [int.from_bytes(rng.bytes(c.Ns), "big") % c.n for _ in range(4)]:
        assert c.mul(k, c.G) == c.mul_affine(k % c.n, c.G), k
        assert c.mul(k, q) == c.mul_affine(k % c.n, q), k
    assert c.mul(5, None) is None


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_mult_rules(curve):
    c = on.CURVES[curve]
    g, zero_row = c.encode(c.G), bytes(c.Ne)
    assert on.scalar_mult(curve, c.sc(1)) == (g, 1)
    assert on.scalar_mult(curve, c.sc(1), None, 1) == (g, 1)
    assert on.scalar_mult(curve, c.sc(0), None, 1) == (zero_row, 0)         # an inverse of zero
    assert on.scalar_mult(curve, c.sc(0), g) == (zero_row, 1)               # 0 P: the identity, a valid result
    assert on.scalar_mult(curve, c.sc(1), zero_row) == (zero_row, 1)        # the identity is accepted here
    p7, _ = on.scalar_mult(curve, c.sc(7), g)
    assert on.scalar_mult(curve, c.sc(7), p7, 1) == (g, 1)
    for bad in (c.n, c.n + 1, 2 ** (8 * c.Ns) - 1):
        assert on.scalar_mult(curve, bad.to_bytes(c.Ns, "big")) == (zero_row, 0)
    assert on.scalar_mult(curve, c.sc(1), b"\x04" + g[1:]) == (zero_row, 0)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_derive_keypair(curve, mode):
    e = entries(curve)[mode]
    sk, pk, ok = on.derive_keypair(curve, mode, hx(e["seed"]), hx(e["keyInfo"]))
    assert (sk.hex(), ok) == (e["skSm"], 1)
    if "pkSm" in e:
        assert pk.hex() == e["pkSm"]
    assert on.scalar_mult(curve, sk)[0] == pk
    assert e["groupDST"] == (b"HashToGroup-" + on.CURVES[curve].context_string(mode)).hex()


@pytest.mark.parametrize("curve", CURVES)
def test_blinded_elements(curve):
    n = 0
    for mode, e in enumerate(entries(curve)):
        for v in e["vectors"]:
            for inp, bl, blinded, _, _ in items(v):
                assert on.blind(curve, mode, inp, bl) == (blinded, 1)
                n += 1
    assert n == 10


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("mode", [0, 1])
def test_evaluations_and_outputs(curve, mode):
    e = entries(curve)[mode]
    sk = hx(e["skSm"])
    for v in e["vectors"]:
        for inp, bl, blinded, evaluated, output in items(v):
            assert on.evaluate(curve, sk, blinded) == (evaluated, 1)
            assert on.finalize(curve, inp, bl, evaluated) == (output, 1)
            assert on.full_evaluate(curve, mode, sk, inp) == (output, 1)


@pytest.mark.parametrize("curve", CURVES)
def test_mode_2_evaluations_through_scalar_mult(curve):
    e = entries(curve)[2]
    n = 0
    for v in e["vectors"]:
        t = on.poprf_scalar(curve, hx(e["skSm"]), hx(v["Info"]))
        for _, _, blinded, evaluated, _ in items(v):
            assert on.scalar_mult(curve, t, blinded, 1) == (evaluated, 1)
            n += 1
    assert n == 4


@pytest.mark.parametrize("curve", CURVES)
def test_failure_rules(curve):
    c = on.CURVES[curve]
    e = entries(curve)[0]
    sk = hx(e["skSm"])
    inp, bl, blinded, evaluated, _ = items(e["vectors"][0])[0]
    for bad in (bytes(c.Ns), c.n.to_bytes(c.Ns, "big"), b"\xff" * c.Ns):
        assert on.blind(curve, 0, inp, bad) == (bytes(c.Ne), 0)
        assert on.evaluate(curve, bad, blinded) == (bytes(c.Ne), 0)
        assert on.finalize(curve, inp, bad, evaluated) == (bytes(c.Nh), 0)
        assert on.full_evaluate(curve, 0, bad, inp) == (bytes(c.Nh), 0)
    for x in (bytes(c.Ne), b"\x04" + blinded[1:], b"\x02" + b"\xff" * c.Ns):
        assert on.evaluate(curve, sk, x) == (bytes(c.Ne), 0)
        assert on.finalize(curve, inp, bl, x) == (bytes(c.Nh), 0)
    long_in = bytes(65536)
    assert on.blind(curve, 0, long_in, bl)[1] == 0 and on.finalize(curve, long_in, bl, evaluated)[1] == 0
    assert on.full_evaluate(curve, 0, sk, long_in)[1] == 0 and on.derive_keypair(curve, 0, bytes(32), long_in)[2] == 0
    assert on.blind(curve, 0, long_in[:-1], bl)[1] == 1


# ---- against the system libcrypto -------------------------------------------------------------------------------------------------
NID = {256: 415, 384: 715}      # NID_X9_62_prime256v1, NID_secp384r1
COMPRESSED = 2                  # POINT_CONVERSION_COMPRESSED


def libcrypto():
    name = ctypes.util.find_library("crypto") or "libcrypto.so.3"
    try:
        L = C.CDLL(name)
        for f in ("EC_GROUP_new_by_curve_name", "EC_POINT_new", "BN_bin2bn", "BN_CTX_new"):
            getattr(L, f).restype = C.c_void_p
        L.EC_GROUP_new_by_curve_name.argtypes = [C.c_int]
        L.EC_POINT_new.argtypes = [C.c_void_p]
        L.BN_bin2bn.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.EC_POINT_mul.argtypes = [C.c_void_p] * 6
        L.EC_POINT_oct2point.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
        L.EC_POINT_point2oct.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p]
        L.EC_POINT_point2oct.restype = C.c_size_t
        for f in ("EC_POINT_free", "EC_GROUP_free", "BN_free", "BN_CTX_free"):
            getattr(L, f).argtypes = [C.c_void_p]
    except (OSError, AttributeError):
        pytest.skip("no libcrypto with EC_POINT_mul on this machine")
    return L


def ec_mul(L, curve, k, elem=None):
    """k G (elem None) or k elem through libcrypto, as a compressed point; the identity as the zero row"""
    c = on.CURVES[curve]
    grp, ctx = L.EC_GROUP_new_by_curve_name(NID[curve]), L.BN_CTX_new()
    assert grp and ctx
    kb = k.to_bytes(c.Ns, "big")
    bn, r, q = L.BN_bin2bn(kb, len(kb), None), L.EC_POINT_new(grp), L.EC_POINT_new(grp)
    try:
        if elem is None:
            assert L.EC_POINT_mul(grp, r, bn, None, None, ctx) == 1
        else:
            assert L.EC_POINT_oct2point(grp, q, elem, len(elem), ctx) == 1
            assert L.EC_POINT_mul(grp, r, None, q, bn, ctx) == 1
        buf = C.create_string_buffer(c.Ne)
        n = L.EC_POINT_point2oct(grp, r, COMPRESSED, buf, c.Ne, ctx)
        return bytes(c.Ne) if n == 1 else buf.raw[:n]       # the identity serialises as the single byte 00
    finally:
        L.EC_POINT_free(r), L.EC_POINT_free(q), L.BN_free(bn), L.BN_CTX_free(ctx), L.EC_GROUP_free(grp)


@pytest.mark.parametrize("curve", CURVES)
def test_checker_equals_libcrypto(curve):
    L = libcrypto()
    c = on.CURVES[curve]
    rng = np.random.default_rng(9497 + curve)
    scalars = list(range(17)) + [c.n - 1, c.n - 2, (c.n + 1) // 2] + [int.from_bytes(rng.bytes(c.Ns), "big") % c.n for _ in range(8)]
    for k in scalars:
        assert on.scalar_mult(curve, c.sc(k)) == (ec_mul(L, curve, k), 1), k
    for i in range(4):
        elem = on.hash_to_group(curve, b"point %d" % i, b"test")
        for k in scalars[::3]:
            assert on.scalar_mult(curve, c.sc(k), elem) == (ec_mul(L, curve, k, elem), 1), (i, k)
    for e in entries(curve)[:2]:            # and libcrypto reproduces the RFC's evaluations
        for v in e["vectors"]:
            for _, _, blinded, evaluated, _ in items(v):
                assert ec_mul(L, curve, int(e["skSm"], 16), blinded) == evaluated
