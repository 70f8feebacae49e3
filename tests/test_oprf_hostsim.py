"""CPU-side checks of the ristretto255 / OPRF device source: ristretto255_dev.h and the item functions of oprf_group_kernels.h compiled for the
host (tests/hostsim/oprf_hostsim.hip) against the checker tests/oprf.py and the fixture, and the same source as a stand-alone program
under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oprf
from conftest import hx, load_golden
from test_oracle_oprf import items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("oprf_ristretto255.json.gz")
SRC = os.path.join(ROOT, "tests", "hostsim", "oprf_hostsim.hip")
vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
H2G, H2S, MULT, DERIVE, BLIND, EVALUATE, FINALIZE, FULL = range(8)      # oprf_group_kernels.h Op
P, L = oprf.P, oprf.L


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
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "liboprf_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_xmd64.argtypes = [vp, vp, u32, vp, u64, vp, u32, vp, u32]
    lib.hs_item.argtypes = [C.c_int, vp, u64]
    for f in ("hs_sqrt_ratio_m1", "hs_mul", "hs_sc_mul"):
        getattr(lib, f).argtypes = [vp, vp, vp]
    for f in ("hs_decode_encode", "hs_map", "hs_from_uniform", "hs_sc_inv", "hs_base"):
        getattr(lib, f).argtypes = [vp, vp]
    lib.hs_equal_identity.argtypes = [vp]
    return lib


def _a(b, dtype=np.uint8):
    """a fresh array holding b (never empty, so that it has an address)"""
    a = np.zeros(max(1, -(-len(b) // np.dtype(dtype).itemsize)), dtype)
    a.view(np.uint8)[:len(b)] = np.frombuffer(b, np.uint8)
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def le(x):
    return x.to_bytes(32, "little")


def call32(fn, *ins, out_words=8):
    """fn(out, *ins) on 32-byte values: (the return value, the output bytes)"""
    out = np.full(out_words + 2, 0xA5A5A5A5, np.uint32)
    arrays = [_a(b, np.uint32) for b in ins]
    rc = fn(_p(out), *[_p(a) for a in arrays])
    assert (out[out_words:] == 0xA5A5A5A5).all()
    return rc, out[:out_words].tobytes()


# ---- the field and group layer ------------------------------------------------------------------------------------------------
def test_sqrt_ratio_m1(hs):
    rng = np.random.default_rng(9496)
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % P
    cases = [(0, 1), (0, 0), (1, 0), (5, 0), (1, 1), (4, 1), (2, 1), (P - 1, 1), (1, P - 1)]
    for _ in range(20):
        x, v = rnd(), rnd()
        cases += [(x * x * v % P, v), (oprf.SQRT_M1 * x * x % P * v % P, v), (rnd(), rnd())]      # a square ratio, a non-square one, any
    seen = set()
    for u, v in cases:
        sq, root = oprf.sqrt_ratio_m1(u, v)
        assert call32(hs.hs_sqrt_ratio_m1, le(u), le(v)) == (int(sq), le(root)), (u, v)
        seen.add(sq)
    assert seen == {True, False}


def test_decode_and_encode_on_the_fixture_lists(hs):
    for k, enc in enumerate(G["multiples"]):
        assert call32(hs.hs_decode_encode, hx(enc)) == (1, hx(enc)), k
        assert call32(hs.hs_base, le(k))[1] == hx(enc), k
        assert hs.hs_equal_identity(_p(_a(hx(enc), np.uint32))) == (k == 0)
    for x in G["invalid"]:
        assert call32(hs.hs_decode_encode, hx(x["enc"]))[0] == 0, x
    rng = np.random.default_rng(1)
    for _ in range(20):     # random bytes: the verdict is the checker's, and what decodes encodes back to itself
        b = rng.bytes(32)
        ok, out = call32(hs.hs_decode_encode, b)
        assert ok == (oprf.decode(b) is not None)
        assert not ok or out == b


def test_elligator_map(hs):
    rng = np.random.default_rng(2)
    special = [0, 1, P - 1, 2, oprf.SQRT_M1, P - oprf.SQRT_M1, 2**255 - 1, P, P + 1]
    for t in special + [int.from_bytes(rng.bytes(32), "little") >> 1 for _ in range(30)]:
        assert call32(hs.hs_map, le(t))[1] == oprf.encode(oprf.elligator(t % P)), t
    t = int.from_bytes(rng.bytes(32), "little") | 1 << 255      # bit 255 is masked
    assert call32(hs.hs_map, le(t))[1] == oprf.encode(oprf.elligator((t & (2**255 - 1)) % P))
    for _ in range(5):
        u = rng.bytes(64)
        t0, t1 = (int.from_bytes(h, "little") & (2**255 - 1) for h in (u[:32], u[32:]))
        assert call32(hs.hs_from_uniform, u)[1] == oprf.encode(oprf.add(oprf.elligator(t0 % P), oprf.elligator(t1 % P)))


@pytest.mark.parametrize("dst_len", [40, 1, 255])
def test_expand_message_xmd_at_every_length(hs, dst_len):
    rng = np.random.default_rng(dst_len)
    dst = (b"HashToGroup-" + oprf.context_string(0)) if dst_len == 40 else rng.bytes(dst_len)
    assert len(dst) == dst_len
    d = _a(dst)
    for n in range(301):
        msg = rng.bytes(n)
        cut1, cut2 = n // 3, n - n // 4       # the three ranges split the message differently at every length
        a, b, c = _a(msg[:cut1]), _a(msg[cut1:cut2]), _a(msg[cut2:])
        out = np.zeros(16, np.uint32)
        hs.hs_xmd64(_p(out), _p(a), cut1, _p(b), cut2 - cut1, _p(c), n - cut2, _p(d), dst_len)
        assert out.tobytes() == oprf.expand_message_xmd(msg, dst), n
    hs.hs_xmd64(_p(out), None, 0, None, 0, None, 0, _p(d), dst_len)
    assert out.tobytes() == oprf.expand_message_xmd(b"", dst)


def test_scalar_inverse_and_product(hs):
    rng = np.random.default_rng(3)
    for x in [1, 2, L - 1, L - 2] + [int.from_bytes(rng.bytes(32), "little") % L for _ in range(12)]:
        _, inv = call32(hs.hs_sc_inv, le(x))
        assert inv == le(pow(x, L - 2, L)), x
        assert call32(hs.hs_sc_mul, le(x), inv)[1] == le(1)
    assert call32(hs.hs_sc_inv, le(0))[1] == le(0)
    a, b = (int.from_bytes(rng.bytes(32), "little") for _ in range(2))      # any 256-bit values
    assert call32(hs.hs_sc_mul, le(a), le(b))[1] == le(a * b % L)


def test_constant_time_multiplication(hs):
    rng = np.random.default_rng(4)
    points = [hx(G["multiples"][1])] + [oprf.hash_to_group(rng.bytes(9), b"test") for _ in range(3)]
    scalars = [0, 1, 2, 8, 15, 16, L - 1] + [int.from_bytes(rng.bytes(32), "little") % L for _ in range(4)]
    for e in points:
        pt = oprf.decode(e)
        for k in scalars:
            assert call32(hs.hs_mul, le(k), e) == (1, oprf.encode(oprf.mul(k, pt))), (e.hex(), k)
    for k in scalars:       # and the comb agrees on the generator
        assert call32(hs.hs_base, le(k))[1] == oprf.encode(oprf.mul(k, oprf.GENERATOR))


# ---- the item functions ---------------------------------------------------------------------------------------------------------
def run_item(hs, op, inp=None, scalar=None, elem=None, seed=None, dst=b"", flags=0, out_bytes=32, two=False):
    """one item through item<op> at index 1 of a batch of 3: (out[, out2], ok); the rows of the neighbours must stay untouched"""
    a = Args()
    keep = []

    def rows(b):
        r = _a(bytes(32) + b + bytes(32), np.uint32)
        keep.append(r)
        return _p(r)

    if inp is not None:
        blob, off = _a(b"ab" + inp + b"c"), np.array([0, 2, 2 + len(inp), 3 + len(inp)], np.uint64)
        keep += [blob, off]
        a.blob, a.off = _p(blob), _p(off)
    if scalar is not None:
        a.scalars, a.scalar_stride = rows(scalar), 8
    if elem is not None:
        a.elems = rows(elem)
    if seed is not None:
        a.seeds = rows(seed)
    out, out2, ok = (np.full(3 * out_bytes // 4, 0xA5A5A5A5, np.uint32) for _ in range(3))
    ok = np.full(3, 7, np.uint8)
    a.out, a.out2, a.ok, a.flags, a.dst_len, a.n = _p(out), _p(out2) if two else None, _p(ok), flags, len(dst), 3
    C.memmove(a.dst, dst, len(dst))
    hs.hs_item(op, C.addressof(a), 1)
    w = out_bytes // 4
    for o in (out, out2) if two else (out,):
        assert (o[:w] == 0xA5A5A5A5).all() and (o[2 * w:] == 0xA5A5A5A5).all()
    assert ok[0] == 7 and ok[2] == 7
    res = (out[w:2 * w].tobytes(),) + ((out2[w:2 * w].tobytes(),) if two else ())
    return res + (int(ok[1]),)


def dst_of(label, mode):
    return label + oprf.context_string(mode)


class Sim:
    """the operations of the C ABI through the item functions: the signatures and results of tests/oprf.py"""

    def __init__(self, hs):
        self.hs = hs

    def hash_to_group(self, msg, dst):
        return run_item(self.hs, H2G, inp=msg, dst=dst)[0]

    def hash_to_scalar(self, msg, dst):
        return run_item(self.hs, H2S, inp=msg, dst=dst)[0]

    def scalar_mult(self, scalar, elem=None, flags=0):
        return run_item(self.hs, MULT, scalar=scalar, elem=elem, flags=flags)

    def derive_keypair(self, mode, seed, info):
        return run_item(self.hs, DERIVE, inp=info, seed=seed, dst=dst_of(b"DeriveKeyPair", mode), two=True)

    def blind(self, mode, inp, bl):
        return run_item(self.hs, BLIND, inp=inp, scalar=bl, dst=dst_of(b"HashToGroup-", mode))

    def evaluate(self, sk, blinded):
        return run_item(self.hs, EVALUATE, scalar=sk, elem=blinded)

    def finalize(self, inp, bl, evaluated):
        return run_item(self.hs, FINALIZE, inp=inp, scalar=bl, elem=evaluated, out_bytes=64)

    def full_evaluate(self, mode, sk, inp):
        return run_item(self.hs, FULL, inp=inp, scalar=sk, dst=dst_of(b"HashToGroup-", mode), out_bytes=64)


def check_fixture(impl):
    """every fixture vector through an implementation of the ABI's operations (the host instantiation here, the GPU in test_gpu_oprf.py)"""
    for k, enc in enumerate(G["multiples"]):
        assert impl.scalar_mult(le(k)) == (hx(enc), 1)
        assert impl.scalar_mult(le(1), hx(enc)) == (hx(enc), 1)
    for x in G["invalid"]:
        assert impl.scalar_mult(le(1), hx(x["enc"])) == (bytes(32), 0), x
    for s in G["scalars"]["valid"]:
        assert impl.scalar_mult(hx(s)) == oprf.scalar_mult(hx(s)) and impl.scalar_mult(hx(s))[1] == 1
    for s in G["scalars"]["invalid"]:
        assert impl.scalar_mult(hx(s)) == (bytes(32), 0), s
    for e in G["rfc9497"]:
        mode, sk = e["mode"], hx(e["skSm"])
        got_sk, got_pk, ok = impl.derive_keypair(mode, hx(e["seed"]), hx(e["keyInfo"]))
        assert (got_sk, ok) == (sk, 1) and got_pk == hx(e.get("pkSm", oprf.scalar_mult(sk)[0].hex()))
        for v in e["vectors"]:
            for inp, bl, blinded, evaluated, output in items(v):
                assert impl.blind(mode, inp, bl) == (blinded, 1)
                assert impl.hash_to_group(inp, hx(e["groupDST"])) == oprf.hash_to_group(inp, hx(e["groupDST"]))
                if mode < 2:
                    assert impl.evaluate(sk, blinded) == (evaluated, 1)
                    assert impl.finalize(inp, bl, evaluated) == (output, 1)
                    assert impl.full_evaluate(mode, sk, inp) == (output, 1)
                else:
                    t = oprf.poprf_scalar(sk, hx(v["Info"]))
                    assert impl.hash_to_scalar(b"Info" + len(hx(v["Info"])).to_bytes(2, "big") + hx(v["Info"]), dst_of(b"HashToScalar-", 2)) == \
                        le((int.from_bytes(t, "little") - int.from_bytes(sk, "little")) % L)
                    assert impl.scalar_mult(t, blinded, 1) == (evaluated, 1)


def test_every_item_function_on_the_fixture(hs):
    check_fixture(Sim(hs))


def test_failure_masks(hs):
    sim = Sim(hs)
    e = G["rfc9497"][0]
    sk = hx(e["skSm"])
    inp, bl, blinded, evaluated, _ = items(e["vectors"][0])[0]
    for bad in (bytes(32), le(L), le(L + 1), b"\xff" * 32):
        assert sim.blind(0, inp, bad) == (bytes(32), 0)
        assert sim.evaluate(bad, blinded) == (bytes(32), 0)
        assert sim.finalize(inp, bad, evaluated) == (bytes(64), 0)
        assert sim.full_evaluate(0, bad, inp) == (bytes(64), 0)
    for x in [bytes(32)] + [hx(x["enc"]) for x in G["invalid"][:6]]:
        assert sim.evaluate(sk, x) == (bytes(32), 0)
        assert sim.finalize(inp, bl, x) == (bytes(64), 0)
    assert sim.scalar_mult(bytes(32), None, 1) == (bytes(32), 0)
    assert sim.scalar_mult(bytes(32), blinded) == (bytes(32), 1)
    assert sim.scalar_mult(le(3), bytes(32)) == (bytes(32), 1)
    long_in = np.random.default_rng(5).bytes(65536)
    assert sim.blind(0, long_in, bl) == (bytes(32), 0)
    assert sim.blind(0, long_in[:-1], bl) == oprf.blind(0, long_in[:-1], bl)
    assert sim.full_evaluate(1, sk, long_in) == (bytes(64), 0)
    assert sim.finalize(long_in, bl, evaluated) == (bytes(64), 0)
    assert sim.derive_keypair(0, sk, long_in) == (bytes(32), bytes(32), 0)
    assert sim.derive_keypair(2, sk, long_in[:-1]) == oprf.derive_keypair(2, sk, long_in[:-1])


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: byte-ragged reads on blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "oprf_hostsim_san"), "-DOPRF_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "oprf_hostsim: ok" in r.stdout, r.stdout[-3000:]
