"""CPU-side checks of the DLEQ / POPRF device source: the element function, both tails and the POPRF item functions of
dleq_group_kernels.h for ristretto255, compiled for the host (tests/hostsim/dleq_hostsim.hip), against the checker tests/dleq.py and the
fixture, and the same source as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dleq
import oprf
from conftest import hx, load_golden
from test_oracle_dleq import CASES, flip
from test_oracle_oprf import items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("oprf_ristretto255.json.gz")
SRC = os.path.join(ROOT, "tests", "hostsim", "dleq_hostsim.hip")
vp, u64, u32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
TWEAK_SERVER, TWEAK_CLIENT, FINALIZE, FULL = range(4)       # dleq_group_kernels.h ItemOp
L = oprf.L


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
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libdleq_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_dleq_request_of.argtypes, lib.hs_dleq_request_of.restype = [vp, u64], u64
    lib.hs_dleq_element.argtypes = [C.c_int, vp, u64, u64, vp, vp]
    lib.hs_dleq_call.argtypes = [C.c_int, vp]
    lib.hs_poprf_item.argtypes = [C.c_int, vp, u64]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _rows(rows, width=32):
    """a fresh word-aligned array holding the rows (never empty, so that it has an address)"""
    a = np.zeros(max(1, len(rows) * width // 4), np.uint32)
    a.view(np.uint8)[:len(rows) * width] = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8)
    return a


def sim_call(hs, verify, ctx, kA, reqs, k=None, r=None, proofs=None, flags=0, div=1, lead=0):
    """One call through the host instantiation.  reqs: a list of (B rows, kB rows); kA / k: one row (shared) or a list (per request).
    div: the offsets' unit (32: bytes, as the host pipeline passes them); lead: elements in front of the first request (a chunk whose
    offsets do not start at 0).  Returns (proof rows, ok) for prove, ok for verify."""
    n_req, shift = len(reqs), {1: 0, 32: 5}[div]
    off = np.array([lead] + [lead + sum(len(b) for b, _ in reqs[:g + 1]) for g in range(n_req)], np.uint64) << np.uint64(shift)
    pad = [bytes(32)] * lead
    B, kB = _rows(pad + [x for b, _ in reqs for x in b]), _rows(pad + [x for _, kb in reqs for x in kb])
    shared = lambda x: isinstance(x, bytes)
    a = Args()
    a.off, a.off_div, a.B, a.kB = _p(off), div, _p(B), _p(kB)
    ka = _rows([kA] if shared(kA) else kA)
    a.kA, a.kA_stride = _p(ka), 0 if shared(kA) else 32
    if not verify:
        kk, rr = _rows([k] if shared(k) else k), _rows(r)
        a.k, a.k_stride, a.r = _p(kk), 0 if shared(k) else 8, _p(rr)
    pr = np.full(16 * n_req + 2, 0xA5A5A5A5, np.uint32)
    if verify:
        pr[:16 * n_req] = _rows(proofs, 64)[:16 * n_req]
    ok, bad = np.full(n_req + 2, 7, np.uint8), np.zeros(max(1, n_req), np.uint32)
    a.proofs, a.ok, a.bad, a.n_req, a.n_elems, a.flags = _p(pr), _p(ok), _p(bad), n_req, int(off[-1] >> np.uint64(shift)) - lead, flags
    tag = b"HashToScalar-" + ctx
    C.memmove(a.tag, tag, len(tag))
    a.tag_len = len(tag)
    hs.hs_dleq_call(int(verify), C.addressof(a))
    assert (pr[16 * n_req:] == 0xA5A5A5A5).all() and (ok[n_req:] == 7).all()
    okl = [int(x) for x in ok[:n_req]]
    if verify:
        return okl
    return [pr[16 * g:16 * g + 16].tobytes() for g in range(n_req)], okl


def test_the_fixture_proofs_in_one_call_per_mode(hs):
    for mode, cases in ((1, CASES[:3]), (2, CASES[3:])):
        ctx = cases[0][1]
        reqs = [(c[4], c[5]) for c in cases]
        ks, kAs, rs, want = [c[2] for c in cases], [c[3] for c in cases], [c[6] for c in cases], [c[7] for c in cases]
        for div, lead in ((1, 0), (32, 0), (32, 3)):
            assert sim_call(hs, False, ctx, kAs, reqs, k=ks, r=rs, flags=1, div=div, lead=lead) == (want, [1, 1, 1]), (mode, div, lead)
            assert sim_call(hs, True, ctx, kAs, reqs, proofs=want, flags=1, div=div, lead=lead) == [1, 1, 1]
        if mode == 1:       # one key for the call
            assert sim_call(hs, False, ctx, kAs[0], reqs, k=ks[0], r=rs) == (want, [1, 1, 1])
        bad = [want[0], flip(want[1], 9), flip(want[2], 300)]
        assert sim_call(hs, True, ctx, kAs, reqs, proofs=bad) == [1, 0, 0]


def test_ragged_requests_against_the_checker(hs):
    """empty requests between others (the search must skip them), j over one byte is left to the GPU tier (the checker's cost)"""
    ctx = b"some other context"
    k, r = (5).to_bytes(32, "little"), [(1000 + g).to_bytes(32, "little") for g in range(6)]
    kA = oprf.scalar_mult(k)[0]
    mult = [oprf.encode(oprf.mul(j, oprf.GENERATOR)) for j in range(1, 9)]
    kmult = [oprf.encode(oprf.mul(5 * j, oprf.GENERATOR)) for j in range(1, 9)]
    sizes = [0, 2, 0, 0, 5, 1]
    reqs, at = [], 0
    for n in sizes:
        reqs.append((mult[at:at + n], kmult[at:at + n]))
        at += n
    want = [dleq.prove(k, kA, b, kb, r[g], ctx) for g, (b, kb) in enumerate(reqs)]
    proofs, ok = sim_call(hs, False, ctx, kA, reqs, k=k, r=r)
    assert ok == [w[1] for w in want] == [0, 1, 0, 0, 1, 1] and proofs == [w[0] for w in want]
    assert sim_call(hs, True, ctx, kA, reqs, proofs=proofs) == [0, 1, 0, 0, 1, 1]
    reqs[4] = (reqs[4][0], reqs[4][1][:3] + [mult[0]] + reqs[4][1][4:])        # another valid element
    assert sim_call(hs, True, ctx, kA, reqs, proofs=proofs) == [0, 1, 0, 0, 0, 1] == \
        [dleq.verify(kA, b, kb, p, ctx) for (b, kb), p in zip(reqs, proofs)]


def test_failure_masks(hs):
    mode, ctx, k, kA, B, kB, r, proof = CASES[2]
    good = (CASES[0][4], CASES[0][5])
    le = lambda x: x.to_bytes(32, "little")

    def prove(k_=k, kA_=kA, B_=B, kB_=kB, r_=r, flags=0):
        # the request under test between two good neighbours (which prove under the same key: the fixture's)
        proofs, ok = sim_call(hs, False, ctx, [kA, kA_, kA], [good, (B_, kB_), good], k=[k, k_, k], r=[CASES[0][6], r_, CASES[0][6]], flags=flags)
        assert ok[0] == ok[2] == 1 and proofs[0] == proofs[2] == CASES[0][7]
        return proofs[1], ok[1]

    assert prove() == (proof, 1)
    for bad in (bytes(32), le(L), le(L + 1), b"\xff" * 32):
        assert prove(k_=bad) == (bytes(64), 0)
        assert prove(r_=bad) == (bytes(64), 0)
    assert prove(kA_=flip(kA)) == (bytes(64), 0)
    assert prove(kB_=[kB[0], flip(kB[1])]) == (bytes(64), 0)
    assert prove(B_=[flip(B[0]), B[1]]) == (bytes(64), 0)
    ident = [bytes(32)]
    assert prove(B_=ident, kB_=ident) == dleq.prove(k, kA, ident, ident, r, ctx) and prove(B_=ident, kB_=ident)[1] == 1
    assert prove(B_=ident, kB_=ident, flags=1) == (bytes(64), 0)
    for part in (0, 32):        # c + L, s + L
        x = int.from_bytes(proof[part:part + 32], "little") + L
        assert sim_call(hs, True, ctx, kA, [good, (B, kB)], proofs=[CASES[0][7], proof[:part] + le(x) + proof[part + 32:]]) == [1, 0]
    assert sim_call(hs, True, ctx, kA, [(B, kB), good], proofs=[proof, CASES[0][7]]) == [1, 1]


# ---- the POPRF items ----------------------------------------------------------------------------------------------------------------
def run_item(hs, op, inp=None, info=None, scalar=None, elem=None, outs=1, out_bytes=32):
    """one item at index 1 of a batch of 3: (out rows..., ok); the rows of the neighbours must stay untouched"""
    a, keep = ItemArgs(), []

    def rag(b):
        blob = np.frombuffer(b"ab" + b + b"c", np.uint8).copy()
        off = np.array([0, 2, 2 + len(b), 3 + len(b)], np.uint64)
        keep.extend([blob, off])
        return _p(blob), _p(off)

    def rows(b):
        r = _rows([bytes(32), b, bytes(32)])
        keep.append(r)
        return _p(r)

    if inp is not None:
        a.input, a.input_off = rag(inp)
    if info is not None:
        a.info, a.info_off = rag(info)
    if scalar is not None:
        a.scalars, a.scalar_stride = rows(scalar), 8
    if elem is not None:
        a.elems, a.elem_stride = rows(elem), 32
    w = out_bytes // 4
    o = [np.full(3 * w, 0xA5A5A5A5, np.uint32) for _ in range(outs)]
    ok = np.full(3, 7, np.uint8)
    a.out, a.ok, a.n = _p(o[0]), _p(ok), 3
    if outs == 3:
        a.out2, a.out3 = _p(o[1]), _p(o[2])
    hs.hs_poprf_item(op, C.addressof(a), 1)
    for x in o:
        assert (x[:w] == 0xA5A5A5A5).all() and (x[2 * w:] == 0xA5A5A5A5).all()
    assert ok[0] == 7 and ok[2] == 7
    return tuple(x[w:2 * w].tobytes() for x in o) + (int(ok[1]),)


def test_poprf_items_on_the_fixture(hs):
    e = G["rfc9497"][2]
    sk, pk = hx(e["skSm"]), hx(e["pkSm"])
    for v in e["vectors"]:
        info = hx(v["Info"])
        want = dleq.poprf_tweak_server(sk, info)
        assert run_item(hs, TWEAK_SERVER, info=info, scalar=sk, outs=3) == want
        assert run_item(hs, TWEAK_CLIENT, info=info, elem=pk) == (want[2], 1)
        for inp, bl, blinded, evaluated, output in items(v):
            assert run_item(hs, FINALIZE, inp=inp, info=info, scalar=bl, elem=evaluated, out_bytes=64) == (output, 1)
            assert run_item(hs, FULL, inp=inp, info=info, scalar=sk, out_bytes=64) == (output, 1)


def test_poprf_failure_masks(hs):
    info = b"some info"
    m = dleq.info_scalar(info)
    le = lambda x: x.to_bytes(32, "little")
    z32, z64 = bytes(32), bytes(64)
    assert run_item(hs, TWEAK_SERVER, info=info, scalar=le(L - m), outs=3) == (z32, z32, z32, 0)
    assert run_item(hs, FULL, inp=b"x", info=info, scalar=le(L - m), out_bytes=64) == (z64, 0)
    minus_mg = oprf.encode(oprf.mul(L - m, oprf.GENERATOR))
    assert run_item(hs, TWEAK_CLIENT, info=info, elem=minus_mg) == (z32, 0)
    assert run_item(hs, TWEAK_CLIENT, info=info, elem=flip(minus_mg)) == (z32, 0)
    for bad in (z32, le(L), b"\xff" * 32):
        assert run_item(hs, TWEAK_SERVER, info=info, scalar=bad, outs=3) == (z32, z32, z32, 0)
        assert run_item(hs, FULL, inp=b"x", info=info, scalar=bad, out_bytes=64) == (z64, 0)
    long_info = np.random.default_rng(6).bytes(65536)
    assert run_item(hs, TWEAK_SERVER, info=long_info, scalar=le(5), outs=3) == (z32, z32, z32, 0)
    assert run_item(hs, TWEAK_SERVER, info=long_info[:-1], scalar=le(5), outs=3) == dleq.poprf_tweak_server(le(5), long_info[:-1])
    assert run_item(hs, TWEAK_CLIENT, info=long_info, elem=minus_mg) == (z32, 0)
    assert run_item(hs, FULL, inp=b"x", info=long_info, scalar=le(5), out_bytes=64) == (z64, 0)
    assert run_item(hs, FULL, inp=long_info, info=info, scalar=le(5), out_bytes=64) == (z64, 0)
    bl, ev = le(9), oprf.encode(oprf.mul(3, oprf.GENERATOR))
    assert run_item(hs, FINALIZE, inp=b"x", info=long_info, scalar=bl, elem=ev, out_bytes=64) == (z64, 0)
    assert run_item(hs, FINALIZE, inp=b"x", info=info, scalar=bl, elem=z32, out_bytes=64) == (z64, 0)
    assert run_item(hs, FINALIZE, inp=b"x", info=None, scalar=bl, elem=ev, out_bytes=64) == dleq.poprf_finalize(b"x", b"", bl, ev)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: element arrays and blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "dleq_hostsim_san"), "-DDLEQ_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "dleq_hostsim: ok" in r.stdout, r.stdout[-3000:]
