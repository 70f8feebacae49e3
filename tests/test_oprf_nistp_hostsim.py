"""CPU-side checks of the P-256 / P-384 device source: nistp_dev.h and the item functions of oprf_group_kernels.h compiled for the host
(tests/hostsim/oprf_nistp_hostsim.hip) against the checker tests/oprf_nistp.py and the fixture, and the same source as a stand-alone
program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oprf_nistp as on
from conftest import hx, load_golden
from test_oracle_oprf_nistp import entries, h2c, items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("oprf_nistp.json.gz")
SRC = os.path.join(ROOT, "tests", "hostsim", "oprf_nistp_hostsim.hip")
vp, u64, u32, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
H2G, H2S, MULT, DERIVE, BLIND, EVALUATE, FINALIZE, FULL = range(8)      # oprf_group_kernels.h Op
CURVES = (256, 384)


class Args(C.Structure):  # oprf_group_kernels.h Args
    _fields_ = [("blob", vp), ("off", vp), ("scalars", vp), ("scalar_stride", C.c_size_t), ("elems", vp), ("seeds", vp), ("out", vp), ("out2", vp),
                ("ok", vp), ("flags", u32), ("dst_len", u32), ("n", C.c_size_t), ("dst", C.c_uint8 * 256)]


def _stale(out):
    from circl_amd import build
    deps = [SRC] + [os.path.join(build.CSRC, h) for h in os.listdir(build.CSRC) if h.endswith(".h")]
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


def _hipcc(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def hs():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "liboprf_nistp_hostsim.so"), "-shared", "-fPIC"))
    for f in ("hs_fe_mul", "hs_add", "hs_mul", "hs_sc_mul"):
        getattr(lib, f).argtypes = [ci, vp, vp, vp]
    for f in ("hs_fe_sqr", "hs_fe_inv", "hs_fe_sqrt", "hs_map", "hs_decode_encode", "hs_dbl", "hs_sc_inv", "hs_reduce_wide_p", "hs_reduce_wide_n"):
        getattr(lib, f).argtypes = [ci, vp, vp]
    lib.hs_fe_addsub.argtypes = [ci, vp, vp, vp, vp]
    lib.hs_sc_is_canonical.argtypes = [ci, vp]
    lib.hs_xmd.argtypes = [ci, vp, u32, vp, u32, vp, u64, vp, u32, vp, u32]
    lib.hs_item.argtypes = [ci, ci, vp, u64]
    return lib


def _a(b):
    """a fresh word-aligned array holding b (never empty, so that it has an address), padded to whole words"""
    a = np.zeros(max(1, -(-len(b) // 4)), np.uint32)
    a.view(np.uint8)[:len(b)] = np.frombuffer(b, np.uint8)
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def call(fn, curve, *ins, out_bytes, outs=1):
    """fn(curve, out..., *ins): (the return value, the output bytes...); the words behind every output must stay untouched"""
    words = -(-out_bytes // 4)
    res = [np.full(words + 2, 0xA5A5A5A5, np.uint32) for _ in range(outs)]
    arrays = [None if b is None else _a(b) for b in ins]
    rc = fn(curve, *[_p(r) for r in res], *[_p(a) for a in arrays])
    for r in res:
        assert (r[words:] == 0xA5A5A5A5).all()
    return (rc,) + tuple(r[:words].tobytes()[:out_bytes] for r in res)


def fe(c, x):
    return x.to_bytes(c.Ns, "big")


def field_values(c, count, seed):
    rng = np.random.default_rng(seed)
    ones = [2 ** (32 * k) - 1 for k in range(1, c.bits // 32)] + [(2 ** 32 - 1) << (c.bits - 64)]          # values with all-ones limbs, below p
    return [0, 1, 2, c.p - 1, c.p - 2] + ones + [int.from_bytes(rng.bytes(c.Ns), "big") % c.p for _ in range(count)]


# ---- the field and scalar layer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_field_arithmetic(hs, curve):
    c = on.CURVES[curve]
    xs = field_values(c, 300, curve)
    assert all(x < c.p for x in xs)
    squares = set()
    for i, x in enumerate(xs):
        y = xs[(7 * i + 3) % len(xs)]
        assert call(hs.hs_fe_mul, curve, fe(c, x), fe(c, y), out_bytes=c.Ns)[1] == fe(c, x * y % c.p), (x, y)
        assert call(hs.hs_fe_sqr, curve, fe(c, x), out_bytes=c.Ns)[1] == fe(c, x * x % c.p), x
        assert call(hs.hs_fe_addsub, curve, fe(c, x), fe(c, y), out_bytes=c.Ns, outs=2)[1:] == (fe(c, (x + y) % c.p), fe(c, (x - y) % c.p)), (x, y)
    for x in xs[:60]:
        assert call(hs.hs_fe_inv, curve, fe(c, x), out_bytes=c.Ns)[1] == fe(c, pow(x, c.p - 2, c.p)), x
        is_sq, root = call(hs.hs_fe_sqrt, curve, fe(c, x), out_bytes=c.Ns)
        assert root == fe(c, pow(x, (c.p + 1) // 4, c.p)) and bool(is_sq) == (pow(x, (c.p - 1) // 2, c.p) in (0, 1)), x
        squares.add(bool(is_sq))
    assert squares == {True, False}


@pytest.mark.parametrize("curve", CURVES)
def test_scalars(hs, curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(3 + curve)
    for x in [1, 2, c.n - 1, c.n - 2] + [int.from_bytes(rng.bytes(c.Ns), "big") % c.n for _ in range(12)]:
        _, inv = call(hs.hs_sc_inv, curve, fe(c, x), out_bytes=c.Ns)
        assert inv == fe(c, pow(x, c.n - 2, c.n)), x
        assert call(hs.hs_sc_mul, curve, fe(c, x), inv, out_bytes=c.Ns)[1] == fe(c, 1)
    assert call(hs.hs_sc_inv, curve, fe(c, 0), out_bytes=c.Ns)[1] == fe(c, 0)
    for x, want in ((0, 1), (c.n - 1, 1), (c.n, 0), (c.n + 1, 0), (2 ** c.bits - 1, 0)):
        assert hs.hs_sc_is_canonical(curve, _p(_a(fe(c, x)))) == want, x


@pytest.mark.parametrize("curve", CURVES)
def test_wide_reductions(hs, curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(5 + curve)
    wide = [bytes(c.ell), b"\xff" * c.ell, fe(c, c.p).rjust(c.ell, b"\0"), fe(c, c.n).rjust(c.ell, b"\0")] + [rng.bytes(c.ell) for _ in range(20)]
    for kind in ("RO", "NU"):       # and the very strings the fixture's u values come from
        f = h2c(curve, kind)
        for v in f["vectors"]:
            count = 2 if kind == "RO" else 1
            u = c.expand_message_xmd(v["msg"].encode(), f["dst"].encode(), count * c.ell)
            for j in range(count):
                w = u[j * c.ell:(j + 1) * c.ell]
                assert int.from_bytes(w, "big") % c.p == int(v["u"][j], 16)
                wide.append(w)
    for w in wide:
        x = int.from_bytes(w, "big")
        assert call(hs.hs_reduce_wide_p, curve, w, out_bytes=c.Ns)[1] == fe(c, x % c.p)
        assert call(hs.hs_reduce_wide_n, curve, w, out_bytes=c.Ns)[1] == fe(c, x % c.n)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("dst_len", [1, 31, 255])
def test_expand_message_xmd_at_every_length(hs, curve, dst_len):
    c = on.CURVES[curve]
    rng = np.random.default_rng(dst_len + curve)
    dst = rng.bytes(dst_len)
    d = _a(dst)
    for n in range(0, 300, 1 if dst_len == 31 else 7):
        msg = rng.bytes(n)
        cut1, cut2 = n // 3, n - n // 4       # the three ranges split the message differently at every length
        a, b, s = _a(msg[:cut1]), _a(msg[cut1:cut2]), _a(msg[cut2:])
        for out_len in (c.ell, 2 * c.ell):
            out = np.zeros(36, np.uint32)
            hs.hs_xmd(curve, _p(out), out_len, _p(a), cut1, _p(b), cut2 - cut1, _p(s), n - cut2, _p(d), dst_len)
            assert out.tobytes()[:out_len] == c.expand_message_xmd(msg, dst, out_len), (n, out_len)


# ---- the group layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_map_to_curve(hs, curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(9380 + curve)
    us = [0, 1, c.p - 1] + [int(x, 16) for kind in ("RO", "NU") for v in h2c(curve, kind)["vectors"] for x in v["u"]]
    us += [int.from_bytes(rng.bytes(c.Ns), "big") % c.p for _ in range(24)]
    seen = set()
    for u in us:
        assert call(hs.hs_map, curve, fe(c, u), out_bytes=c.Ne)[1] == c.encode(c.map_to_curve(u)), u
        seen.add(c.sswu_branch(u))
    assert seen == {(True, 0), (True, 1), (False, 0), (False, 1)}       # both sides of e2, both signs
    for kind in ("RO", "NU"):
        for v in h2c(curve, kind)["vectors"]:
            qs = [v["Q0"], v["Q1"]] if kind == "RO" else [v["Q"]]
            for u, q in zip(v["u"], qs):
                assert call(hs.hs_map, curve, fe(c, int(u, 16)), out_bytes=c.Ne)[1] == c.encode((int(q["x"], 16), int(q["y"], 16)))


@pytest.mark.parametrize("curve", CURVES)
def test_complete_addition_and_generator_multiples(hs, curve):
    c = on.CURVES[curve]
    g, zero = c.encode(c.G), bytes(c.Ne)
    neg_g = c.encode(c.neg(c.G))
    assert call(hs.hs_add, curve, g, g, out_bytes=c.Ne) == (1, c.encode(c.add(c.G, c.G)))          # P + P
    assert call(hs.hs_dbl, curve, g, out_bytes=c.Ne) == (1, c.encode(c.add(c.G, c.G)))
    assert call(hs.hs_add, curve, g, neg_g, out_bytes=c.Ne) == (1, zero)                           # P + (-P)
    assert call(hs.hs_add, curve, g, zero, out_bytes=c.Ne) == (1, g)                               # P + identity
    assert call(hs.hs_add, curve, zero, g, out_bytes=c.Ne) == (1, g)
    assert call(hs.hs_add, curve, zero, zero, out_bytes=c.Ne) == (1, zero)                         # identity + identity
    assert call(hs.hs_dbl, curve, zero, out_bytes=c.Ne) == (1, zero)
    rng = np.random.default_rng(6 + curve)
    pts = [c.mul(int.from_bytes(rng.bytes(8), "big"), c.G) for _ in range(4)]
    for p in pts:
        for q in pts:
            assert call(hs.hs_add, curve, c.encode(p), c.encode(q), out_bytes=c.Ne) == (1, c.encode(c.add(p, q)))
    for k in list(range(17)) + [c.n - 1, c.n - 2, (c.n + 1) // 2]:
        assert call(hs.hs_mul, curve, fe(c, k), None, out_bytes=c.Ne) == (1, c.encode(c.mul(k, c.G))), k
    e = c.encode(pts[0])
    for k in (0, 1, 2, c.n - 1, int.from_bytes(rng.bytes(c.Ns), "big") % c.n):
        assert call(hs.hs_mul, curve, fe(c, k), e, out_bytes=c.Ne) == (1, c.encode(c.mul(k, pts[0]))), k


def bad_encodings(c):
    """rows that must not decode: x = p, p + 1, 2^(8 Ns) - 1, a non-residue x, and the prefixes 00, 04, 05 on a good x"""
    gx = fe(c, c.G[0])
    x = next(x for x in range(2, 100) if c.decode(b"\x02" + fe(c, x)) is False)
    return [b"\x02" + fe(c, c.p), b"\x03" + fe(c, c.p + 1), b"\x02" + b"\xff" * c.Ns, b"\x02" + fe(c, x), b"\x03" + fe(c, x),
            b"\x00" + gx, b"\x04" + gx, b"\x05" + gx]


@pytest.mark.parametrize("curve", CURVES)
def test_strict_decoding(hs, curve):
    c = on.CURVES[curve]
    for b in bad_encodings(c):
        assert c.decode(b) is False
        assert call(hs.hs_decode_encode, curve, b, out_bytes=c.Ne)[0] == 0, b.hex()
    rng = np.random.default_rng(1 + curve)
    seen = set()
    for _ in range(30):     # random x: the verdict is the checker's, and what decodes encodes back to itself
        b = bytes([2 + int(rng.integers(2))]) + fe(c, int.from_bytes(rng.bytes(c.Ns), "big") % c.p)
        ok, out = call(hs.hs_decode_encode, curve, b, out_bytes=c.Ne)
        assert ok == (c.decode(b) is not False) and (not ok or out == b)
        seen.add(ok)
    assert seen == {0, 1}
    assert call(hs.hs_decode_encode, curve, bytes(c.Ne), out_bytes=c.Ne) == (1, bytes(c.Ne))


# ---- the item functions ---------------------------------------------------------------------------------------------------------
def run_item(hs, curve, op, inp=None, scalar=None, elem=None, seed=None, dst=b"", flags=0, out_bytes=32, out2_bytes=0):
    """one item through Item<op> at index 1 of a batch of 3: (out[, out2], ok); the rows of the neighbours must stay untouched"""
    a = Args()
    keep = []

    def rows(b):
        r = _a(bytes(len(b)) + b + bytes(len(b)))
        keep.append(r)
        return _p(r)

    if inp is not None:
        blob, off = np.frombuffer(b"ab" + inp + b"c", np.uint8).copy(), np.array([0, 2, 2 + len(inp), 3 + len(inp)], np.uint64)
        keep += [blob, off]
        a.blob, a.off = _p(blob), _p(off)
    if scalar is not None:
        a.scalars, a.scalar_stride = rows(scalar), len(scalar) // 4
    if elem is not None:
        a.elems = rows(elem)
    if seed is not None:
        a.seeds = rows(seed)
    out, out2 = np.full(3 * out_bytes + 4, 0xA5, np.uint8), np.full(3 * max(out2_bytes, 1) + 4, 0xA5, np.uint8)
    ok = np.full(3, 7, np.uint8)
    a.out, a.out2, a.ok, a.flags, a.dst_len, a.n = _p(out), _p(out2) if out2_bytes else None, _p(ok), flags, len(dst), 3
    C.memmove(a.dst, dst, len(dst))
    hs.hs_item(curve, op, C.addressof(a), 1)
    res = []
    for o, w in ((out, out_bytes), (out2, out2_bytes)):
        if w:
            assert (o[:w] == 0xA5).all() and (o[2 * w:] == 0xA5).all()
            res.append(o[w:2 * w].tobytes())
    assert ok[0] == 7 and ok[2] == 7
    return tuple(res) + (int(ok[1]),)


class Sim:
    """the operations of the C ABI through the item functions: the signatures and results of tests/oprf_nistp.py"""

    def __init__(self, hs):
        self.hs = hs

    def hash_to_group(self, curve, msg, dst, flags=0):
        return run_item(self.hs, curve, H2G, inp=msg, dst=dst, flags=flags, out_bytes=on.CURVES[curve].Ne)[0]

    def hash_to_scalar(self, curve, msg, dst):
        return run_item(self.hs, curve, H2S, inp=msg, dst=dst, out_bytes=on.CURVES[curve].Ns)[0]

    def scalar_mult(self, curve, scalar, elem=None, flags=0):
        return run_item(self.hs, curve, MULT, scalar=scalar, elem=elem, flags=flags, out_bytes=on.CURVES[curve].Ne)

    def derive_keypair(self, curve, mode, seed, info):
        c = on.CURVES[curve]
        return run_item(self.hs, curve, DERIVE, inp=info, seed=seed, dst=b"DeriveKeyPair" + c.context_string(mode), out_bytes=c.Ns, out2_bytes=c.Ne)

    def blind(self, curve, mode, inp, bl):
        c = on.CURVES[curve]
        return run_item(self.hs, curve, BLIND, inp=inp, scalar=bl, dst=b"HashToGroup-" + c.context_string(mode), out_bytes=c.Ne)

    def evaluate(self, curve, sk, blinded):
        return run_item(self.hs, curve, EVALUATE, scalar=sk, elem=blinded, out_bytes=on.CURVES[curve].Ne)

    def finalize(self, curve, inp, bl, evaluated):
        return run_item(self.hs, curve, FINALIZE, inp=inp, scalar=bl, elem=evaluated, out_bytes=on.CURVES[curve].Nh)

    def full_evaluate(self, curve, mode, sk, inp):
        c = on.CURVES[curve]
        return run_item(self.hs, curve, FULL, inp=inp, scalar=sk, dst=b"HashToGroup-" + c.context_string(mode), out_bytes=c.Nh)


def check_fixture(impl, curve):
    """every fixture vector of a curve through an implementation of the ABI's operations (the host instantiation here, the GPU in
    test_gpu_oprf_nistp.py), bit-exact"""
    c = on.CURVES[curve]
    for kind in ("RO", "NU"):
        f = h2c(curve, kind)
        for v in f["vectors"]:
            want = c.encode((int(v["P"]["x"], 16), int(v["P"]["y"], 16)))
            assert impl.hash_to_group(curve, v["msg"].encode(), f["dst"].encode(), int(kind == "NU")) == want, (kind, v["msg"])
    for e in entries(curve):
        mode, sk = e["mode"], hx(e["skSm"])
        got_sk, got_pk, ok = impl.derive_keypair(curve, mode, hx(e["seed"]), hx(e["keyInfo"]))
        assert (got_sk, ok) == (sk, 1) and got_pk == hx(e.get("pkSm", on.scalar_mult(curve, sk)[0].hex()))
        assert impl.scalar_mult(curve, sk) == (got_pk, 1)
        for v in e["vectors"]:
            for inp, bl, blinded, evaluated, output in items(v):
                assert impl.blind(curve, mode, inp, bl) == (blinded, 1)
                if mode < 2:
                    assert impl.evaluate(curve, sk, blinded) == (evaluated, 1)
                    assert impl.finalize(curve, inp, bl, evaluated) == (output, 1)
                    assert impl.full_evaluate(curve, mode, sk, inp) == (output, 1)
                else:
                    info = hx(v["Info"])
                    t = on.poprf_scalar(curve, sk, info)
                    assert impl.hash_to_scalar(curve, b"Info" + len(info).to_bytes(2, "big") + info, b"HashToScalar-" + c.context_string(2)) == \
                        c.sc(int.from_bytes(t, "big") - int.from_bytes(sk, "big"))
                    assert impl.scalar_mult(curve, t, blinded, 1) == (evaluated, 1)


@pytest.mark.parametrize("curve", CURVES)
def test_every_item_function_on_the_fixture(hs, curve):
    check_fixture(Sim(hs), curve)


@pytest.mark.parametrize("curve", CURVES)
def test_failure_masks(hs, curve):
    sim, c = Sim(hs), on.CURVES[curve]
    e = entries(curve)[0]
    sk = hx(e["skSm"])
    inp, bl, blinded, evaluated, _ = items(e["vectors"][0])[0]
    for bad in (bytes(c.Ns), fe(c, c.n), fe(c, c.n + 1), b"\xff" * c.Ns):
        assert sim.blind(curve, 0, inp, bad) == (bytes(c.Ne), 0)
        assert sim.evaluate(curve, bad, blinded) == (bytes(c.Ne), 0)
        assert sim.finalize(curve, inp, bad, evaluated) == (bytes(c.Nh), 0)
        assert sim.full_evaluate(curve, 0, bad, inp) == (bytes(c.Nh), 0)
    for x in [bytes(c.Ne)] + bad_encodings(c):
        assert sim.evaluate(curve, sk, x) == (bytes(c.Ne), 0)
        assert sim.finalize(curve, inp, bl, x) == (bytes(c.Nh), 0)
    for x in bad_encodings(c):
        assert sim.scalar_mult(curve, fe(c, 1), x) == (bytes(c.Ne), 0)
    assert sim.scalar_mult(curve, bytes(c.Ns), None, 1) == (bytes(c.Ne), 0)            # an inverse of zero
    assert sim.scalar_mult(curve, bytes(c.Ns), blinded) == (bytes(c.Ne), 1)            # identity out
    assert sim.scalar_mult(curve, fe(c, 3), bytes(c.Ne)) == (bytes(c.Ne), 1)           # identity in
    for bad in (c.n, c.n + 1, 2 ** c.bits - 1):
        assert sim.scalar_mult(curve, fe(c, bad)) == (bytes(c.Ne), 0)
    long_in = np.random.default_rng(5).bytes(65536)
    assert sim.blind(curve, 0, long_in, bl) == (bytes(c.Ne), 0)
    assert sim.blind(curve, 0, long_in[:-1], bl) == on.blind(curve, 0, long_in[:-1], bl)
    assert sim.full_evaluate(curve, 1, sk, long_in) == (bytes(c.Nh), 0)
    assert sim.finalize(curve, long_in, bl, evaluated) == (bytes(c.Nh), 0)
    assert sim.derive_keypair(curve, 0, bytes(32), long_in) == (bytes(c.Ns), bytes(c.Ne), 0)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: byte-ragged reads on blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "oprf_nistp_hostsim_san"), "-DOPRF_NISTP_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "oprf_nistp_hostsim: ok" in r.stdout, r.stdout[-3000:]
