"""GPU tests of the batch DLEQ proofs on P-256 / P-384 (circl_hip_nistp_dleq_*) and the mode-2 OPRF items (circl_hip_oprf_nistp_poprf_*),
both forms of every entry point on both curves, and of the verifiable protocol compositions of the wrappers, against the CPU checker
tests/dleq_nistp.py and the fixture.  Every output lies between guard margins that must survive.  The sizes are those at which the
segmented reduction can go wrong (request edges on and off wavefront edges, many requests in a wave, requests over several waves, a
partial last wave), not workload sizes.  Elements are B_j = b_j G with known b_j: the expected proof of a request then costs the
checker one multiplication by sum d_j b_j instead of one per element."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dleq_nistp as dn
import oprf_nistp as on
from conftest import hx
from test_oracle_dleq_nistp import CASES, entries, flip, items

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
CURVES = (256, 384)
FORMS = [(c, f) for c in CURVES for f in ("host", "dev")]
SMALL = 15      # the distinct elements of the long requests: j G for j = 1 .. 15


def rows(x, width):
    if isinstance(x, (list, tuple)):
        x = b"".join(bytes(r) for r in x)
    a = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8).reshape(-1, width)
    return a if len(a) else np.zeros((1, width), np.uint8)


class Out:
    def __init__(self, *shape):
        self.shape, self.nbytes = shape, int(np.prod(shape))


class Form:
    """the C ABI of one curve through ctypes, on host buffers or on device tensors: inputs are numpy arrays (None: a NULL pointer), outputs
    are allocated here between guard margins, checked and returned as numpy arrays.  On the device every ELEMENT array is placed at an odd
    address."""

    def __init__(self, curve, kind):
        from circl_amd import _native as nat
        from circl_amd import build as cbuild
        cbuild.build()
        self.nat, self.lib, self.dev, self.curve, self.c = nat, nat.lib(), kind == "dev", curve, on.CURVES[curve]
        self.Ns, self.Ne, self.Nh = self.c.Ns, self.c.Ne, self.c.Nh

    def run(self, entry, args, counts, host=(), odd=()):
        """counts: what follows the arguments (n, or n_req and n_elems); host: indices of arguments that stay host bytes in both forms; odd:
        indices of element arrays (inputs and outputs), which the dev form places at odd addresses"""
        import torch
        keep, outs, cargs = [], [], []
        for i, a in enumerate(args):
            shift = 1 if (self.dev and i in odd) else 0
            if isinstance(a, Out):
                if self.dev:
                    t = torch.full((a.nbytes + 2 * GUARD + 1,), FILL, dtype=torch.uint8, device="cuda")
                    cargs.append(C.c_void_p(t.data_ptr() + GUARD + shift))
                else:
                    t = np.full(a.nbytes + 2 * GUARD + 1, FILL, np.uint8)
                    cargs.append(C.c_void_p(t.ctypes.data + GUARD))
                outs.append((t, a, shift))
            elif isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                if self.dev and i not in host:
                    flat = a.view(np.uint8).reshape(-1)
                    t = torch.from_numpy(np.concatenate([np.full(shift, FILL, np.uint8), flat])).cuda()
                    keep.append(t)
                    cargs.append(C.c_void_p(t.data_ptr() + shift))
                else:
                    keep.append(a)
                    cargs.append(a.ctypes.data_as(C.c_void_p))
            else:
                cargs.append(a)
        dleq = entry.startswith("nistp_dleq")
        if self.dev and dleq:
            wsb = self.lib.circl_hip_nistp_dleq_workspace_size(self.curve, *counts)
            ws = torch.full((wsb + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")       # (torch's blocks are 256-byte aligned)
            assert GUARD % 8 == 0
            tail = (*counts, C.c_void_p(ws.data_ptr() + GUARD), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        elif self.dev:
            tail = (counts[0], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            tail = (counts[0], 0)
        self.nat.check(getattr(self.lib, "circl_hip_" + entry + ("_dev" if self.dev else ""))(self.curve, *cargs, *tail), entry)
        if self.dev and dleq:
            torch.cuda.synchronize()
            w = ws.cpu().numpy()
            assert (w[:GUARD] == FILL).all() and (w[GUARD + wsb:] == FILL).all(), entry + ": the workspace's margins"
        res = []
        for t, a, shift in outs:
            if self.dev:
                torch.cuda.synchronize()
                t = t.cpu().numpy()
            lo = GUARD + shift
            assert (t[:lo] == FILL).all() and (t[lo + a.nbytes:] == FILL).all(), entry
            res.append(t[lo:lo + a.nbytes].reshape(a.shape).copy())
        return res

    @staticmethod
    def blob(items_):
        if items_ is None:
            return None, None
        off = np.zeros(len(items_) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in items_])
        return np.frombuffer(b"".join(items_) + bytes(16), np.uint8).copy(), off

    def _key(self, x, width):
        """(rows, stride): bytes = one row for the call"""
        return (rows(x, width), 0) if isinstance(x, bytes) else (rows(x, width), width)

    def prove(self, k, kA, B, kB, off, r, ctx, flags=0):
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        dst = np.frombuffer(ctx + b"\0", np.uint8)
        args = [*self._key(k, self.Ns), *self._key(kA, self.Ne), rows(B, self.Ne), rows(kB, self.Ne), off, rows(r, self.Ns), dst, len(ctx), flags,
                Out(n, 2 * self.Ns), Out(n)]
        return self.run("nistp_dleq_prove", args, (n, int(off[-1] - off[0])), host=(8,), odd=(2, 4, 5))

    def verify(self, kA, B, kB, off, proofs, ctx, flags=0):
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        dst = np.frombuffer(ctx + b"\0", np.uint8)
        args = [*self._key(kA, self.Ne), rows(B, self.Ne), rows(kB, self.Ne), off, rows(proofs, 2 * self.Ns), dst, len(ctx), flags, Out(n)]
        return self.run("nistp_dleq_verify", args, (n, int(off[-1] - off[0])), host=(6,), odd=(0, 2, 3))[0]

    def tweak_server(self, sk, infos):
        n = len(infos)
        return self.run("oprf_nistp_poprf_tweak", [*self._key(sk, self.Ns), None, 0, *self.blob(infos), Out(n, self.Ns), Out(n, self.Ns), Out(n, self.Ne), Out(n)],
                        (n,), odd=(8,))

    def tweak_client(self, pk, infos):
        n = len(infos)
        return self.run("oprf_nistp_poprf_tweak", [None, 0, *self._key(pk, self.Ne), *self.blob(infos), None, None, Out(n, self.Ne), Out(n)], (n,), odd=(2, 8))

    def poprf_finalize(self, inputs, infos, blinds, evaluated):
        n = len(inputs)
        return self.run("oprf_nistp_poprf_finalize", [*self.blob(inputs), *self.blob(infos), rows(blinds, self.Ns), rows(evaluated, self.Ne), Out(n, self.Nh), Out(n)],
                        (n,), odd=(5,))

    def poprf_full_evaluate(self, sk, inputs, infos):
        n = len(inputs)
        return self.run("oprf_nistp_poprf_full_evaluate", [*self._key(sk, self.Ns), *self.blob(inputs), *self.blob(infos), Out(n, self.Nh), Out(n)], (n,))

    def evaluate(self, sk, blinded):
        n = len(rows(blinded, self.Ne))
        return self.run("oprf_nistp_evaluate", [*self._key(sk, self.Ns), rows(blinded, self.Ne), Out(n, self.Ne), Out(n)], (n,))


_forms = {}


@pytest.fixture(params=FORMS, ids=lambda p: "P%d-%s" % p)
def form(request):
    if request.param not in _forms:
        _forms[request.param] = Form(*request.param)
    return _forms[request.param]


def offsets(sizes, first=0):
    off = np.full(len(sizes) + 1, first, np.uint64)
    off[1:] += np.cumsum(sizes).astype(np.uint64)
    return off


_small = {}


def small(curve, k=1):
    """the encodings of k j G for j = 0 .. SMALL (index 0: the identity's zero row), computed once per curve and key"""
    if (curve, k) not in _small:
        c = on.CURVES[curve]
        _small[curve, k] = [bytes(c.Ne)] + [c.encode(c.mul(k * j % c.n, c.G)) for j in range(1, SMALL + 1)]
    return _small[curve, k]


def scalar_ints(rng, c, n):
    return [1 + int.from_bytes(rng.bytes(c.Ns), "big") % (c.n - 1) for _ in range(n)]


_expected = {}


def expected(c, k, r, kA, bs, ctx):
    """the proof of one request whose pairs are (b G, k b G) for b in bs, in closed form; k, r integers.  Computed once for both forms."""
    key = (c.bits, k, r, ctx, tuple(bs))
    if key not in _expected:
        enc_b, enc_kb = small(c.bits), small(c.bits, k)
        seed = dn.seed_of(c, kA, ctx)
        total = sum(dn.composite_scalar(c, seed, j, enc_b[b], enc_kb[b], ctx) * b for j, b in enumerate(bs)) % c.n
        _expected[key] = dn.proof_from(c, k, r, kA, c.mul(total, c.G), ctx)
    return _expected[key]


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_proofs_in_one_call_per_mode(form):
    cases_all = CASES[form.curve]
    for cases in (cases_all[:3], cases_all[3:]):
        ctx = cases[0][1]
        off = offsets([len(c[4]) for c in cases])
        assert list(np.diff(off.astype(np.int64))) == [1, 1, 2]
        B, kB = [x for c in cases for x in c[4]], [x for c in cases for x in c[5]]
        k, kA, r, want = [c[2] for c in cases], [c[3] for c in cases], [c[6] for c in cases], [c[7] for c in cases]
        proofs, ok = form.prove(k, kA, B, kB, off, r, ctx, 1)
        assert [p.tobytes() for p in proofs] == want and ok.tolist() == [1, 1, 1]
        assert form.verify(kA, B, kB, off, want, ctx, 1).tolist() == [1, 1, 1]
        assert form.verify(kA, B, kB, off, [want[0], flip(want[1], 77), want[2]], ctx, 1).tolist() == [1, 0, 1]


def test_mode_2_outputs_on_the_fixture(form):
    e = entries(form.curve)[2]
    sk, pk = hx(e["skSm"]), hx(e["pkSm"])
    its = [(hx(v["Info"]),) + it for v in e["vectors"] for it in items(v)]
    assert len(its) == 4
    infos, inputs, blinds = [i[0] for i in its], [i[1] for i in its], [i[2] for i in its]
    t, tinv, tg, ok = form.tweak_server(sk, infos)
    want = [dn.poprf_tweak_server(form.curve, sk, info) for info in infos]
    assert ok.all() and [(a.tobytes(), b.tobytes(), c.tobytes(), 1) for a, b, c in zip(t, tinv, tg)] == want
    tw, ok = form.tweak_client(pk, infos)
    assert ok.all() and (tw == tg).all()
    evaluated, ok = form.evaluate(tinv, [i[3] for i in its])
    assert ok.all() and [x.tobytes() for x in evaluated] == [i[4] for i in its]
    out, ok = form.poprf_finalize(inputs, infos, blinds, evaluated)
    assert ok.all() and [x.tobytes() for x in out] == [i[5] for i in its]
    out, ok = form.poprf_full_evaluate(sk, inputs, infos)
    assert ok.all() and [x.tobytes() for x in out] == [i[5] for i in its]
    out, ok = form.poprf_full_evaluate([sk] * 4, inputs, infos)         # a key per item
    assert ok.all() and [x.tobytes() for x in out] == [i[5] for i in its]


# ---- 2. segment shapes ----------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 61, 1, 63, 64, 65, 1, 1, 128, 300, 3]


def segment_inputs(c, sizes, keys):
    """(bs per request, B rows, kB rows) for requests of these sizes, request g under keys[g]"""
    bs, at = [], 0
    for n in sizes:
        bs.append([1 + (7 * j + j // SMALL) % SMALL for j in range(at, at + n)])
        at += n
    B = [small(c.bits)[b] for req in bs for b in req]
    kB = [small(c.bits, keys[g])[b] for g, req in enumerate(bs) for b in req]
    return bs, B, kB


@pytest.mark.parametrize("keying", ["one-key", "key-per-request"])
def test_segment_shapes(form, keying):
    c, ctx = form.c, b"segment shapes"
    rng = np.random.default_rng(11 + c.bits)
    n = len(SIZES)
    one = keying == "one-key"
    keys = scalar_ints(rng, c, 1) * n if one else scalar_ints(rng, c, n)
    rs = scalar_ints(rng, c, n)
    kAs = [c.encode(c.mul(k, c.G)) for k in keys]
    bs, B, kB = segment_inputs(c, SIZES, keys)
    assert len(B) == 690
    off = offsets(SIZES)
    k_arg, kA_arg = (c.sc(keys[0]), kAs[0]) if one else ([c.sc(k) for k in keys], kAs)
    proofs, ok = form.prove(k_arg, kA_arg, B, kB, off, [c.sc(r) for r in rs], ctx)
    assert ok.all()
    for g in range(n):
        assert proofs[g].tobytes() == expected(c, keys[g], rs[g], kAs[g], bs[g], ctx), (g, SIZES[g])
    assert form.verify(kA_arg, B, kB, off, proofs, ctx).tolist() == [1] * n


def test_an_empty_request_between_two_live_ones_and_offsets_that_start_late(form):
    c, ctx = form.c, b"ragged"
    rng = np.random.default_rng(21 + c.bits)
    sizes = [70, 0, 5, 0, 0, 64]
    n = len(sizes)
    (key,), rs = scalar_ints(rng, c, 1), scalar_ints(rng, c, n)
    kA = c.encode(c.mul(key, c.G))
    bs, B, kB = segment_inputs(c, sizes, [key] * n)
    want = [expected(c, key, rs[g], kA, bs[g], ctx) if sizes[g] else bytes(2 * c.Ns) for g in range(n)]
    live = [int(s > 0) for s in sizes]
    proofs, ok = form.prove(c.sc(key), kA, B, kB, offsets(sizes), [c.sc(r) for r in rs], ctx)
    assert ok.tolist() == live and [p.tobytes() for p in proofs] == want
    pr = [w if l else want[0] for w, l in zip(want, live)]
    assert form.verify(kA, B, kB, offsets(sizes), pr, ctx).tolist() == live
    if form.dev:        # req_off[0] != 0: B and kB are indexed by the absolute element, 37 rows lie in front
        lead = [small(c.bits)[3]] * 37
        proofs, ok = form.prove(c.sc(key), kA, lead + B, lead + kB, offsets(sizes, 37), [c.sc(r) for r in rs], ctx)
        assert ok.tolist() == live and [p.tobytes() for p in proofs] == want
        assert form.verify(kA, lead + B, lead + kB, offsets(sizes, 37), pr, ctx).tolist() == live


# ---- 3. tampering ---------------------------------------------------------------------------------------------------------------
def test_tampering_leaves_the_neighbours_alone(form):
    c, ctx = form.c, b"tampering"
    rng = np.random.default_rng(12 + c.bits)
    sizes = [3, 130, 2]
    off = offsets(sizes)
    (key,), rs = scalar_ints(rng, c, 1), scalar_ints(rng, c, 3)
    kA = c.encode(c.mul(key, c.G))
    bs, B, kB = segment_inputs(c, sizes, [key] * 3)
    proofs, ok = form.prove(c.sc(key), kA, B, kB, off, [c.sc(r) for r in rs], ctx)
    assert ok.all() and form.verify(kA, B, kB, off, proofs, ctx).tolist() == [1, 1, 1]

    def case(kA_=None, kB_=None, B_=None, proof_=None):
        pr = proofs.copy()
        if proof_ is not None:
            pr[1] = np.frombuffer(proof_, np.uint8)
        assert form.verify([kA, kA_ or kA, kA], B_ or B, kB_ or kB, off, pr, ctx).tolist() == [1, 0, 1]

    for j in (0, 63, 64, 129):                  # one flipped bit (the other y) in kB: first / last lane of a wave, first of the next, last
        t = list(kB)
        t[3 + j] = flip(t[3 + j])
        case(kB_=t)
    t = list(kB)
    t[3 + 17] = flip(t[3 + 17], 8 * c.Ne - 3)   # one flipped bit of x: on the curve or not, the request fails
    case(kB_=t)
    t, u = list(kB), list(B)                    # two pairs swapped: the index j is bound
    assert B[3 + 5] != B[3 + 70]
    t[3 + 5], t[3 + 70], u[3 + 5], u[3 + 70] = t[3 + 70], t[3 + 5], u[3 + 70], u[3 + 5]
    case(kB_=t, B_=u)
    p = proofs[1].tobytes()
    case(proof_=flip(p, 6))                     # c
    case(proof_=flip(p, 8 * c.Ns + 6))          # s
    case(kA_=c.encode(c.mul(key + 1, c.G)))     # another valid key
    case(kA_=b"\x04" + kA[1:])                  # does not decode


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------
def test_limits_of_a_request(form):
    """65535 pairs pass, 65536 and 0 fail, and the neighbours are untouched"""
    c, ctx = form.c, b"limits"
    key, rs = 0x1234567, [77, 0x7654321, 78, 79, 80]
    kA = c.encode(c.mul(key, c.G))
    sizes = [2, 65535, 65536, 0, 2]
    off = offsets(sizes)
    bs = [[1, 5], [3] * 65535, [3] * 65536, [], [3, 5]]
    B = rows([small(c.bits)[b] for req in bs for b in req], c.Ne)
    kB = rows([small(c.bits, key)[b] for req in bs for b in req], c.Ne)
    proofs, ok = form.prove(c.sc(key), kA, B, kB, off, [c.sc(r) for r in rs], ctx)
    assert ok.tolist() == [1, 1, 0, 0, 1]
    assert not proofs[2].any() and not proofs[3].any()
    for g in (0, 1, 4):
        assert proofs[g].tobytes() == expected(c, key, rs[g], kA, bs[g], ctx), g
    pr = proofs.copy()
    pr[2], pr[3] = proofs[1], proofs[0]     # well-formed proofs: the requests fail for their sizes
    assert form.verify(kA, B, kB, off, pr, ctx).tolist() == [1, 1, 0, 0, 1]


# ---- 5. masks -------------------------------------------------------------------------------------------------------------------
def test_failure_masks(form):
    c, ctx, curve = form.c, b"masks", form.curve
    rng = np.random.default_rng(13 + curve)
    (key,) = scalar_ints(rng, c, 1)
    k, good_r, kA = c.sc(key), c.sc(4242), c.encode(c.mul(key, c.G))
    pair = lambda j: (small(curve)[j], small(curve, key)[j])
    base = [pair(1 + j % SMALL) for j in range(70)]
    bad_prefix, big_x, off_curve = list(base), list(base), list(base)
    bad_prefix[35] = (base[35][0], b"\x04" + base[35][1][1:])
    big_x[69] = (b"\x02" + b"\xff" * c.Ns, base[69][1])
    off_curve[0] = (next(x for x in (b"\x03" + c.sc(v)[-c.Ns:] for v in range(1, 50)) if c.decode(x) is False), base[0][1])
    ident = [pair(2), pair(0), pair(3)]
    be = lambda x: x.to_bytes(c.Ns, "big")
    # (k, kA, r, pairs) -- every bad request between good ones
    reqs = [
        (k, kA, good_r, base[:2]),
        (k, kA, bytes(c.Ns), base[:2]), (k, kA, be(c.n), base[:2]), (k, kA, b"\xff" * c.Ns, base[:2]),
        (bytes(c.Ns), kA, good_r, base[:2]), (be(c.n + 5), kA, good_r, base[:2]),
        (k, kA, good_r, base),
        (k, kA, good_r, bad_prefix), (k, kA, good_r, big_x), (k, kA, good_r, off_curve),
        (k, b"\x05" + kA[1:], good_r, base[:3]),
        (k, kA, good_r, ident),
        (k, kA, good_r, base[:2]),
    ]
    off = offsets([len(q[3]) for q in reqs])
    B, kB = [p[0] for q in reqs for p in q[3]], [p[1] for q in reqs for p in q[3]]
    ks, kAs, rs = [q[0] for q in reqs], [q[1] for q in reqs], [q[2] for q in reqs]
    for flags in (0, 1):
        want = [dn.prove(curve, q[0], q[1], [p[0] for p in q[3]], [p[1] for p in q[3]], q[2], ctx, flags) for q in reqs]
        assert [w[1] for w in want] == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 - flags, 1]
        proofs, ok = form.prove(ks, kAs, B, kB, off, rs, ctx, flags)
        assert ok.tolist() == [w[1] for w in want]
        assert [p.tobytes() for p in proofs] == [w[0] for w in want]
        # the verifier on the same requests, each with a proof that is good for its elements where one exists
        pr = [w[0] if w[1] else want[0][0] for w in want]
        verdict = form.verify(kAs, B, kB, off, pr, ctx, flags).tolist()
        assert verdict == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1 - flags, 1]      # (requests 1 .. 5 are request 0 under a bad k or r: its proof verifies)
    # c or s >= n, each between two good requests
    p0 = want[0][0]
    for bad in (be(c.n) + p0[c.Ns:], p0[:c.Ns] + be(c.n + 1), b"\xff" * c.Ns + p0[c.Ns:], p0[:c.Ns] + b"\xff" * c.Ns):
        o3 = offsets([2, 2, 2])
        assert form.verify(kA, B[:2] * 3, kB[:2] * 3, o3, [p0, bad, p0], ctx).tolist() == [1, 0, 1]


def test_poprf_failure_masks(form):
    c, curve = form.c, form.curve
    info = b"some info"
    m = dn.info_scalar(c, info)
    long_info = np.random.default_rng(6).bytes(65536)
    infos = [info, info, long_info, long_info[:-1], b""]
    sks = [c.sc(5), c.sc(c.n - m), c.sc(5), c.sc(5), c.sc(5)]            # the second: t = 0 (sk = -m)
    want = [dn.poprf_tweak_server(curve, s, i) for s, i in zip(sks, infos)]
    t, tinv, tg, ok = form.tweak_server(sks, infos)
    assert ok.tolist() == [1, 0, 0, 1, 1] == [w[3] for w in want]
    assert [(a.tobytes(), b.tobytes(), x.tobytes()) for a, b, x in zip(t, tinv, tg)] == [w[:3] for w in want]
    minus_mg = c.encode(c.mul(c.n - m, c.G))
    g4 = small(curve)[4]
    pks = [g4, minus_mg, g4, g4, b"\x04" + g4[1:]]                       # the second lands on the identity
    want = [dn.poprf_tweak_client(curve, p, i) for p, i in zip(pks, infos)]
    tw, ok = form.tweak_client(pks, infos)
    assert ok.tolist() == [1, 0, 0, 1, 0] == [w[1] for w in want] and [x.tobytes() for x in tw] == [w[0] for w in want]
    inputs = [b"x", b"y", b"z", b"", long_info]
    want = [dn.poprf_full_evaluate(curve, s, x, i) for s, x, i in zip(sks, inputs, infos)]
    out, ok = form.poprf_full_evaluate(sks, inputs, infos)
    assert ok.tolist() == [1, 0, 0, 1, 0] == [w[1] for w in want] and [x.tobytes() for x in out] == [w[0] for w in want]
    blinds, ev = [c.sc(9)] * 5, [small(curve)[3]] * 3 + [bytes(c.Ne), small(curve)[3]]
    want = [dn.poprf_finalize(curve, x, i, b, e) for x, i, b, e in zip(inputs, infos, blinds, ev)]
    out, ok = form.poprf_finalize(inputs, infos, blinds, ev)
    assert ok.tolist() == [1, 1, 0, 0, 0] == [w[1] for w in want] and [x.tobytes() for x in out] == [w[0] for w in want]
    out, ok = form.poprf_finalize(inputs[:2], None, blinds[:2], ev[:2])     # no infos: every item's is empty
    assert [(x.tobytes(), 1) for x in out] == [dn.poprf_finalize(curve, x, b"", b, e) for x, b, e in zip(inputs, blinds, ev)][:2]


# ---- 6. the host pipeline's routes ----------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 requests at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices


@pytest.mark.parametrize("curve", CURVES)
def test_pipeline_routes_agree(curve, tmp_path):
    from circl_amd import hostapi as api
    import dleq_nistp_worker as dw
    c = on.CURVES[curve]
    base = dw.run(api, curve, 0, N_PIPE)
    assert base["ok"].all() and base["verdict"].all()
    assert base["verdict_bad"].tolist() == [1 - g % 2 for g in range(N_PIPE)]
    for key in ("ok_tw", "ok_tw1", "ok_twc", "ok_pfin", "ok_pfin0", "ok_pfull", "ok_pfull0"):
        assert base[key].all(), key
    assert (base["twc"] == base["tw1"]).all()         # pk + m G = (sk + m) G
    k, kA, B, kB, off, r, b = dw.inputs(api, curve, N_PIPE)
    infos, ins = dw.item_inputs(N_PIPE)
    by = lambda a: a.tobytes()
    for g in (0, 99, 100, 255, 256, 299):             # both ends, both sides of a shard boundary and of the chunk boundary
        lo, hi = int(off[g]), int(off[g + 1])
        assert by(base["proofs"][g]) == dn.prove(curve, by(k[g]), by(kA[g]), [by(x) for x in B[lo:hi]], [by(x) for x in kB[lo:hi]], by(r[g]), dw.CTX, 1)[0], g
        assert (by(base["t"][g]), by(base["tinv"][g]), by(base["tw"][g]), 1) == dn.poprf_tweak_server(curve, by(k[g]), infos[g]), g
        assert by(base["pfin"][g]) == dn.poprf_finalize(curve, ins[g], infos[g], by(r[g]), by(kA[g]))[0], g
        assert by(base["pfin0"][g]) == dn.poprf_finalize(curve, ins[g], b"", by(r[g]), by(kA[g]))[0], g
        assert by(base["pfull"][g]) == dn.poprf_full_evaluate(curve, by(k[g]), ins[g], infos[g])[0], g
        assert by(base["pfull0"][g]) == dn.poprf_full_evaluate(curve, by(k[0]), ins[g], b"")[0], g
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dleq_nistp_worker.py")
    for env, device in (({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1)):
        dst = str(tmp_path / ("out%d.npz" % device))
        e = {k_: v for k_, v in os.environ.items() if k_ not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
        e.update(env)
        subprocess.run([sys.executable, worker, str(curve), str(device), str(N_PIPE), dst], check=True, env=e, timeout=300)
        o = np.load(dst)
        for key in base:
            assert (np.asarray(o[key]) == base[key]).all(), (key, env)


# ---- 7. the protocol through the wrappers ---------------------------------------------------------------------------------------
class HostWrappers:
    def __init__(self, curve):
        from circl_amd import hostapi as api
        self.o, self.c = api.NistpOprf(curve), on.CURVES[curve]

    def blind(self, mode, inputs, blinds):
        return self.o.blind(mode, inputs, rows(blinds, self.c.Ns))

    def evaluate_verifiable(self, mode, sk, blinded, off, r, info):
        return self.o.evaluate_verifiable(mode, sk, blinded, off, rows(r, self.c.Ns), info)

    def finalize_verifiable(self, mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info):
        return self.o.finalize_verifiable(mode, pk, inputs, rows(blinds, self.c.Ns), blinded, evaluated, off, proofs, info)

    def full_evaluate(self, mode, sk, inputs, info):
        if mode == 1:
            return self.o.full_evaluate(1, sk, inputs)
        return self.o.poprf_full_evaluate(sk, inputs, [info] * len(inputs))

    def public_key(self, sk):
        return self.o.scalar_mult(sk, n=1)[0][0].tobytes()


class DeviceWrappers:
    def __init__(self, curve):
        import torch
        from circl_amd import device as dev
        self.torch, self.dev, self.o, self.c = torch, dev, dev.NistpOprfDevice(curve), on.CURVES[curve]

    def t(self, x, width):
        return self.torch.from_numpy(rows(x, width).copy()).cuda()

    def blind(self, mode, inputs, blinds):
        out, ok = self.o.blind(mode, self.dev.Ragged(inputs), self.t(blinds, self.c.Ns))
        return out.cpu().numpy(), ok.cpu().numpy()

    def evaluate_verifiable(self, mode, sk, blinded, off, r, info):
        c = self.c
        return tuple(x.cpu().numpy() for x in self.o.evaluate_verifiable(mode, self.t(sk, c.Ns), self.t(blinded, c.Ne), off, self.t(r, c.Ns), info))

    def finalize_verifiable(self, mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info):
        c = self.c
        return tuple(x.cpu().numpy() for x in self.o.finalize_verifiable(mode, self.t(pk, c.Ne), self.dev.Ragged(inputs), self.t(blinds, c.Ns), self.t(blinded, c.Ne),
                                                                         self.t(evaluated, c.Ne), off, self.t(proofs, 2 * c.Ns), info))

    def full_evaluate(self, mode, sk, inputs, info):
        n = len(inputs)
        if mode == 1:
            out, ok = self.o.full_evaluate(1, self.t(sk, self.c.Ns), self.dev.Ragged(inputs), n)
        else:
            out, ok = self.o.poprf_full_evaluate(self.t(sk, self.c.Ns), self.dev.Ragged(inputs), self.dev.Ragged([info] * n), n)
        return out.cpu().numpy(), ok.cpu().numpy()

    def public_key(self, sk):
        return self.o.scalar_mult(self.t(sk, self.c.Ns), n=1)[0].cpu().numpy()[0].tobytes()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("curve,kind", FORMS)
def test_protocol_round_trip(curve, kind, mode):
    c = on.CURVES[curve]
    w = HostWrappers(curve) if kind == "host" else DeviceWrappers(curve)
    rng = np.random.default_rng(14 + mode + curve)
    sizes, info = [1, 2, 70], b"public info" if mode == 2 else b""
    off, n_el = offsets(sizes), sum(sizes)
    sk, other = (c.sc(x) for x in scalar_ints(rng, c, 2))
    pk = w.public_key(sk)
    assert pk == c.encode(c.mul(int.from_bytes(sk, "big"), c.G))
    inputs = [rng.bytes(j % 9) for j in range(n_el)]
    blinds, r = [c.sc(x) for x in scalar_ints(rng, c, n_el)], [c.sc(x) for x in scalar_ints(rng, c, 3)]
    blinded, ok = w.blind(mode, inputs, blinds)
    assert ok.all()
    evaluated, proofs, ok = w.evaluate_verifiable(mode, sk, blinded, off, r, info)
    assert ok.tolist() == [1, 1, 1]
    out, ok = w.finalize_verifiable(mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info)
    full, full_ok = w.full_evaluate(mode, sk, inputs, info)
    assert ok.tolist() == [1, 1, 1] and full_ok.all() and (out == full).all() and out.any(axis=1).all()
    # the checker on the first request, both ends
    want = on.full_evaluate(curve, 1, sk, inputs[0]) if mode == 1 else dn.poprf_full_evaluate(curve, sk, inputs[0], info)
    assert (out[0].tobytes(), 1) == want
    # one evaluated element of the middle request replaced by another valid element
    bad = evaluated.copy()
    bad[2] = evaluated[0]
    out2, ok2 = w.finalize_verifiable(mode, pk, inputs, blinds, blinded, bad, off, proofs, info)
    assert ok2.tolist() == [1, 0, 1]
    assert not out2[1:3].any() and (out2[0] == out[0]).all() and (out2[3:] == out[3:]).all()
    # a client that holds another key refuses everything
    out3, ok3 = w.finalize_verifiable(mode, w.public_key(other), inputs, blinds, blinded, evaluated, off, proofs, info)
    assert ok3.tolist() == [0, 0, 0] and not out3.any()
