"""CPU-side checks of the NIST-curve DLEQ / POPRF device source: the element function, both tails and the POPRF item functions of
dleq_group_kernels.h compiled for the host (tests/hostsim/dleq_nistp_hostsim.hip) against the checker tests/dleq_nistp.py and the
fixture, on both curves, and the same source as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dleq_nistp as dn
import oprf_nistp as on
from conftest import hx
from test_oracle_dleq_nistp import CASES, entries, flip, items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "dleq_nistp_hostsim.hip")
vp, u64, u32, sz, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t, C.c_int
TWEAK_SERVER, TWEAK_CLIENT, FINALIZE, FULL = range(4)       # dleq_group_kernels.h ItemOp
CURVES = (256, 384)


class Args(C.Structure):  # dleq_group_kernels.h Args
    _fields_ = [("off", vp), ("off_div", u32), ("B", vp), ("kB", vp), ("k", vp), ("k_stride", sz), ("kA", vp), ("kA_stride", sz), ("r", vp),
                ("proofs", vp), ("ok", vp), ("partial", vp), ("bad", vp), ("n_req", sz), ("n_elems", sz), ("flags", u32), ("tag_len", u32),
                ("tag", C.c_uint8 * 256)]


class ItemArgs(C.Structure):  # dleq_group_kernels.h ItemArgs
    _fields_ = [("input", vp), ("input_off", vp), ("info", vp), ("info_off", vp), ("scalars", vp), ("scalar_stride", sz), ("elems", vp),
                ("elem_stride", sz), ("out", vp), ("out2", vp), ("out3", vp), ("ok", vp), ("n", sz)]


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
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libdleq_nistp_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_nistp_dleq_request_of.argtypes, lib.hs_nistp_dleq_request_of.restype = [ci, vp, u64], u64
    lib.hs_nistp_dleq_element.argtypes = [ci, ci, vp, u64, u64, vp, vp]
    lib.hs_nistp_dleq_call.argtypes = [ci, ci, vp]
    lib.hs_nistp_poprf_item.argtypes = [ci, ci, vp, u64]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _words(rows, width):
    """a fresh word-aligned array holding the rows (never empty, so that it has an address)"""
    a = np.zeros(max(1, len(rows) * width // 4), np.uint32)
    a.view(np.uint8)[:len(rows) * width] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8)
    return a


def _packed(rows, width):
    """packed byte rows that begin at an odd address: (the array that owns them, their address)"""
    a = np.zeros(len(rows) * width + 1, np.uint8)
    a[1:] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8)
    return a, a.ctypes.data + 1


def sim_call(hs, curve, verify, ctx, kA, reqs, k=None, r=None, proofs=None, flags=0, div=1, lead=0):
    """One call through the host instantiation.  reqs: a list of (B rows, kB rows); kA / k: one row (shared) or a list (per request).
    div: the offsets' unit (Ne: bytes, as the host pipeline passes them); lead: elements in front of the first request (a chunk whose
    offsets do not start at 0).  Returns (proof rows, ok) for prove, ok for verify."""
    c = on.CURVES[curve]
    n_req, pw = len(reqs), c.Ns // 2
    off = np.array([lead] + [lead + sum(len(b) for b, _ in reqs[:g + 1]) for g in range(n_req)], np.uint64) * np.uint64(div)
    pad = [bytes(c.Ne)] * lead
    (B, pB), (kB, pkB) = _packed(pad + [x for b, _ in reqs for x in b], c.Ne), _packed(pad + [x for _, kb in reqs for x in kb], c.Ne)
    shared = lambda x: isinstance(x, bytes)
    a = Args()
    a.off, a.off_div, a.B, a.kB = _p(off), div, pB, pkB
    ka, pka = _packed([kA] if shared(kA) else kA, c.Ne)
    a.kA, a.kA_stride = pka, 0 if shared(kA) else c.Ne
    if not verify:
        kk, rr = _words([k] if shared(k) else k, c.Ns), _words(r, c.Ns)
        a.k, a.k_stride, a.r = _p(kk), 0 if shared(k) else c.Ns // 4, _p(rr)
    pr = np.full(pw * n_req + 2, 0xA5A5A5A5, np.uint32)
    if verify:
        pr[:pw * n_req] = _words(proofs, 2 * c.Ns)[:pw * n_req]
    ok, bad = np.full(n_req + 2, 7, np.uint8), np.zeros(max(1, n_req), np.uint32)
    a.proofs, a.ok, a.bad, a.n_req, a.n_elems, a.flags = _p(pr), _p(ok), _p(bad), n_req, int(off[-1]) // div - lead, flags
    tag = b"HashToScalar-" + ctx
    C.memmove(a.tag, tag, len(tag))
    a.tag_len = len(tag)
    hs.hs_nistp_dleq_call(curve, int(verify), C.addressof(a))
    assert (pr[pw * n_req:] == 0xA5A5A5A5).all() and (ok[n_req:] == 7).all()
    okl = [int(x) for x in ok[:n_req]]
    if verify:
        return okl
    return [pr[pw * g:pw * g + pw].tobytes() for g in range(n_req)], okl


@pytest.mark.parametrize("curve", CURVES)
def test_the_fixture_proofs_in_one_call_per_mode(hs, curve):
    ne = on.CURVES[curve].Ne
    for mode, cases in ((1, CASES[curve][:3]), (2, CASES[curve][3:])):
        ctx = cases[0][1]
        reqs = [(c[4], c[5]) for c in cases]
        ks, kAs, rs, want = [c[2] for c in cases], [c[3] for c in cases], [c[6] for c in cases], [c[7] for c in cases]
        for div, lead in ((1, 0), (ne, 0), (ne, 3)):
            assert sim_call(hs, curve, False, ctx, kAs, reqs, k=ks, r=rs, flags=1, div=div, lead=lead) == (want, [1, 1, 1]), (mode, div, lead)
            assert sim_call(hs, curve, True, ctx, kAs, reqs, proofs=want, flags=1, div=div, lead=lead) == [1, 1, 1]
        if mode == 1:       # one key for the call
            assert sim_call(hs, curve, False, ctx, kAs[0], reqs, k=ks[0], r=rs) == (want, [1, 1, 1])
        bad = [want[0], flip(want[1], 9), flip(want[2], 8 * ne + 70)]
        assert sim_call(hs, curve, True, ctx, kAs, reqs, proofs=bad) == [1, 0, 0]


@pytest.mark.parametrize("curve", CURVES)
def test_ragged_requests_against_the_checker(hs, curve):
    """empty requests between others (the search must skip them); j over one byte is left to the GPU tier (the checker's cost)"""
    c = on.CURVES[curve]
    ctx = b"some other context"
    k, r = c.sc(5), [c.sc(1000 + g) for g in range(6)]
    kA = c.encode(c.mul(5, c.G))
    mult = [c.encode(c.mul(j, c.G)) for j in range(1, 9)]
    kmult = [c.encode(c.mul(5 * j, c.G)) for j in range(1, 9)]
    sizes = [0, 2, 0, 0, 5, 1]
    reqs, at = [], 0
    for n in sizes:
        reqs.append((mult[at:at + n], kmult[at:at + n]))
        at += n
    want = [dn.prove(curve, k, kA, b, kb, r[g], ctx) for g, (b, kb) in enumerate(reqs)]
    proofs, ok = sim_call(hs, curve, False, ctx, kA, reqs, k=k, r=r)
    assert ok == [w[1] for w in want] == [0, 1, 0, 0, 1, 1] and proofs == [w[0] for w in want]
    assert sim_call(hs, curve, True, ctx, kA, reqs, proofs=proofs) == [0, 1, 0, 0, 1, 1]
    reqs[4] = (reqs[4][0], reqs[4][1][:3] + [mult[0]] + reqs[4][1][4:])        # another valid element
    assert sim_call(hs, curve, True, ctx, kA, reqs, proofs=proofs) == [0, 1, 0, 0, 0, 1] == \
        [dn.verify(curve, kA, b, kb, p, ctx) for (b, kb), p in zip(reqs, proofs)]
    # the search over the offsets, in both units
    off = np.array([0, 0, 2, 2, 2, 7, 8], np.uint64)
    for div in (1, c.Ne):
        a = Args()
        scaled = off * np.uint64(div)
        a.off, a.off_div, a.n_req = _p(scaled), div, 6
        assert [hs.hs_nistp_dleq_request_of(curve, C.addressof(a), e) for e in range(8)] == [1, 1, 4, 4, 4, 4, 4, 5]


@pytest.mark.parametrize("curve", CURVES)
def test_failure_masks(hs, curve):
    c = on.CURVES[curve]
    mode, ctx, k, kA, B, kB, r, proof = CASES[curve][2]
    first = CASES[curve][0]
    good = (first[4], first[5])
    zero = (bytes(2 * c.Ns), 0)
    be = lambda x: x.to_bytes(c.Ns, "big")

    def prove(k_=k, kA_=kA, B_=B, kB_=kB, r_=r, flags=0):
        # the request under test between two good neighbours (which prove under the same key: the fixture's)
        proofs, ok = sim_call(hs, curve, False, ctx, [kA, kA_, kA], [good, (B_, kB_), good], k=[k, k_, k], r=[first[6], r_, first[6]], flags=flags)
        assert ok[0] == ok[2] == 1 and proofs[0] == proofs[2] == first[7]
        return proofs[1], ok[1]

    assert prove() == (proof, 1)
    for bad in (bytes(c.Ns), be(c.n), be(c.n + 1), b"\xff" * c.Ns):
        assert prove(k_=bad) == zero
        assert prove(r_=bad) == zero
    assert prove(kA_=b"\x04" + kA[1:]) == zero                                  # a bad prefix
    assert prove(kB_=[kB[0], b"\x02" + b"\xff" * c.Ns]) == zero                 # x >= p
    off_curve = next(x for x in (b"\x02" + be(v) for v in range(1, 50)) if c.decode(x) is False)
    assert prove(B_=[off_curve, B[1]]) == zero                                  # not on the curve
    ident = [bytes(c.Ne)]
    assert prove(B_=ident, kB_=ident) == dn.prove(curve, k, kA, ident, ident, r, ctx) and prove(B_=ident, kB_=ident)[1] == 1
    assert prove(B_=ident, kB_=ident, flags=1) == zero
    for part in (0, c.Ns):        # c + n, s + n (where that still fits the row), and all ones
        for x in (int.from_bytes(proof[part:part + c.Ns], "big") + c.n, 2 ** (8 * c.Ns) - 1):
            if x < 2 ** (8 * c.Ns):
                assert sim_call(hs, curve, True, ctx, kA, [good, (B, kB)], proofs=[first[7], proof[:part] + be(x) + proof[part + c.Ns:]]) == [1, 0]
    assert sim_call(hs, curve, True, ctx, kA, [(B, kB), good], proofs=[proof, first[7]]) == [1, 1]
    assert sim_call(hs, curve, True, ctx, kA, [(B, [flip(kB[0]), kB[1]]), good], proofs=[proof, first[7]]) == [0, 1]      # one flipped bit


def test_element_function(hs):
    """d_j B_j of one lane against the checker, as projective words"""
    for curve in CURVES:
        c = on.CURVES[curve]
        mode, ctx, k, kA, B, kB, r, proof = CASES[curve][2]
        n = c.Ns // 4
        off = np.array([0, 2], np.uint64)
        (bB, pB), (bkB, pkB), (bkA, pkA) = _packed(B, c.Ne), _packed(kB, c.Ne), _packed([kA], c.Ne)
        a = Args()
        a.off, a.off_div, a.B, a.kB, a.kA, a.n_req, a.n_elems = _p(off), 1, pB, pkB, pkA, 1, 2
        tag = b"HashToScalar-" + ctx
        C.memmove(a.tag, tag, len(tag))
        a.tag_len = len(tag)
        seed = dn.seed_of(c, kA, ctx)
        R = pow(2, 32 * n, c.p)
        for j in range(2):
            m, z = np.zeros(3 * n, np.uint32), np.zeros(3 * n, np.uint32)
            assert hs.hs_nistp_dleq_element(curve, 1, C.addressof(a), 0, j, _p(m), _p(z)) == 1
            d = dn.composite_scalar(c, seed, j, B[j], kB[j], ctx)
            for words, row in ((m, B[j]), (z, kB[j])):
                X, Y, Z = (int.from_bytes(words[i * n:(i + 1) * n].tobytes(), "little") * pow(R, -1, c.p) % c.p for i in range(3))
                zi = pow(Z, -1, c.p)
                assert (X * zi % c.p, Y * zi % c.p) == c.mul(d, c.decode(row))


# ---- the POPRF items ----------------------------------------------------------------------------------------------------------------
def run_item(hs, curve, op, inp=None, info=None, scalar=None, elem=None):
    """one item at index 1 of a batch of 3: (out rows..., ok); the rows of the neighbours must stay untouched"""
    c = on.CURVES[curve]
    a, keep = ItemArgs(), []

    def rag(b):
        blob = np.frombuffer(b"ab" + b + b"c", np.uint8).copy()
        off = np.array([0, 2, 2 + len(b), 3 + len(b)], np.uint64)
        keep.extend([blob, off])
        return _p(blob), _p(off)

    if inp is not None:
        a.input, a.input_off = rag(inp)
    if info is not None:
        a.info, a.info_off = rag(info)
    if scalar is not None:
        s = _words([bytes(c.Ns), scalar, bytes(c.Ns)], c.Ns)
        keep.append(s)
        a.scalars, a.scalar_stride = _p(s), c.Ns // 4
    if elem is not None:
        e, pe = _packed([bytes(c.Ne), elem, bytes(c.Ne)], c.Ne)
        keep.append(e)
        a.elems, a.elem_stride = pe, c.Ne
    widths = {TWEAK_SERVER: (c.Ns, c.Ns, c.Ne), TWEAK_CLIENT: (c.Ne,), FINALIZE: (c.Nh,), FULL: (c.Nh,)}[op]
    outs = []
    for wd in widths:      # word rows are word-aligned; element rows begin at an odd address
        buf = np.full(3 * wd + 8, 0xA5, np.uint8)
        at = (-buf.ctypes.data) % 4 + (1 if wd == c.Ne else 0)
        outs.append((buf, at, wd))
    ok = np.full(3, 7, np.uint8)
    ptrs = [b.ctypes.data + at for b, at, _ in outs]
    a.out, a.ok, a.n = ptrs[0], _p(ok), 3
    if len(outs) == 3:
        a.out2, a.out3 = ptrs[1], ptrs[2]
    hs.hs_nistp_poprf_item(curve, op, C.addressof(a), 1)
    res = []
    for b, at, wd in outs:
        assert (b[:at + wd] == 0xA5).all() and (b[at + 2 * wd:] == 0xA5).all()
        res.append(b[at + wd:at + 2 * wd].tobytes())
    assert ok[0] == 7 and ok[2] == 7
    return tuple(res) + (int(ok[1]),)


@pytest.mark.parametrize("curve", CURVES)
def test_poprf_items_on_the_fixture(hs, curve):
    e = entries(curve)[2]
    sk, pk = hx(e["skSm"]), hx(e["pkSm"])
    for v in e["vectors"]:
        info = hx(v["Info"])
        want = dn.poprf_tweak_server(curve, sk, info)
        assert run_item(hs, curve, TWEAK_SERVER, info=info, scalar=sk) == want
        assert run_item(hs, curve, TWEAK_CLIENT, info=info, elem=pk) == (want[2], 1)
        for inp, bl, blinded, evaluated, output in items(v):
            assert run_item(hs, curve, FINALIZE, inp=inp, info=info, scalar=bl, elem=evaluated) == (output, 1)
            assert run_item(hs, curve, FULL, inp=inp, info=info, scalar=sk) == (output, 1)


@pytest.mark.parametrize("curve", CURVES)
def test_poprf_failure_masks(hs, curve):
    c = on.CURVES[curve]
    info = b"some info"
    m = dn.info_scalar(c, info)
    zs, ze, zh = bytes(c.Ns), bytes(c.Ne), bytes(c.Nh)
    assert run_item(hs, curve, TWEAK_SERVER, info=info, scalar=c.sc(c.n - m)) == (zs, zs, ze, 0)          # t = 0
    assert run_item(hs, curve, FULL, inp=b"x", info=info, scalar=c.sc(c.n - m)) == (zh, 0)
    minus_mg = c.encode(c.mul(c.n - m, c.G))
    assert run_item(hs, curve, TWEAK_CLIENT, info=info, elem=minus_mg) == (ze, 0)                         # lands on the identity
    assert run_item(hs, curve, TWEAK_CLIENT, info=info, elem=flip(minus_mg)) == dn.poprf_tweak_client(curve, flip(minus_mg), info)
    assert run_item(hs, curve, TWEAK_CLIENT, info=info, elem=b"\x05" + minus_mg[1:]) == (ze, 0)
    for bad in (zs, c.n.to_bytes(c.Ns, "big"), b"\xff" * c.Ns):
        assert run_item(hs, curve, TWEAK_SERVER, info=info, scalar=bad) == (zs, zs, ze, 0)
        assert run_item(hs, curve, FULL, inp=b"x", info=info, scalar=bad) == (zh, 0)
    long_info = np.random.default_rng(6).bytes(65536)
    assert run_item(hs, curve, TWEAK_SERVER, info=long_info, scalar=c.sc(5)) == (zs, zs, ze, 0)
    assert run_item(hs, curve, TWEAK_SERVER, info=long_info[:-1], scalar=c.sc(5)) == dn.poprf_tweak_server(curve, c.sc(5), long_info[:-1])
    assert run_item(hs, curve, TWEAK_CLIENT, info=long_info, elem=minus_mg) == (ze, 0)
    assert run_item(hs, curve, FULL, inp=b"x", info=long_info, scalar=c.sc(5)) == (zh, 0)
    assert run_item(hs, curve, FULL, inp=long_info, info=info, scalar=c.sc(5)) == (zh, 0)
    bl, ev = c.sc(9), c.encode(c.mul(3, c.G))
    assert run_item(hs, curve, FINALIZE, inp=b"x", info=long_info, scalar=bl, elem=ev) == (zh, 0)
    assert run_item(hs, curve, FINALIZE, inp=b"x", info=info, scalar=bl, elem=ze) == (zh, 0)
    assert run_item(hs, curve, FINALIZE, inp=b"x", info=None, scalar=bl, elem=ev) == dn.poprf_finalize(curve, b"x", b"", bl, ev)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: element arrays and blobs of exactly their size, at odd addresses"""
    exe = _hipcc(os.path.join(ROOT, "build", "dleq_nistp_hostsim_san"), "-DDLEQ_NISTP_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "dleq_nistp_hostsim: ok" in r.stdout, r.stdout[-3000:]
