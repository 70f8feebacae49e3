"""GPU tests of the batch DLEQ proofs (circl_hip_dleq_*) and the mode-2 OPRF items (circl_hip_oprf_poprf_*), both forms of every entry
point, and of the verifiable protocol compositions of the wrappers, against the CPU checker tests/dleq.py and the fixture.  Every
output lies between guard margins that must survive.  The sizes are those at which the segmented reduction can go wrong (request
edges on and off wavefront edges, many requests in a wave, requests over several waves, a partial last wave), not workload sizes.
Elements are small multiples of the generator: the checker multiplies once per DISTINCT element of a request."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dleq
import oprf
from conftest import hx, load_golden
from test_oracle_dleq import CASES, flip
from test_oracle_oprf import items

pytestmark = pytest.mark.gpu

G = load_golden("oprf_ristretto255.json.gz")
GUARD, FILL = 64, 0xA5
L = oprf.L
FORMS = ["host", "dev"]
MULT = [hx(x) for x in G["multiples"]]      # j G for j = 0 .. 15


def le(x):
    return x.to_bytes(32, "little")


def rows(x, width=32):
    if isinstance(x, (list, tuple)):
        x = b"".join(bytes(r) for r in x)
    a = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8).reshape(-1, width)
    return a if len(a) else np.zeros((1, width), np.uint8)


class Out:
    def __init__(self, *shape):
        self.shape, self.nbytes = shape, int(np.prod(shape))


class Form:
    """the C ABI through ctypes, on host buffers or on device tensors: inputs are numpy arrays (None: a NULL pointer), outputs are allocated
    here between guard margins, checked and returned as numpy arrays"""

    def __init__(self, kind):
        from circl_amd import _native as nat
        from circl_amd import build as cbuild
        cbuild.build()
        self.nat, self.lib, self.dev = nat, nat.lib(), kind == "dev"

    def run(self, entry, args, counts, host=()):
        """counts: what follows the arguments (n, or n_req and n_elems); host: indices of arguments that stay host bytes in both forms"""
        import torch
        keep, outs, cargs = [], [], []
        for i, a in enumerate(args):
            if isinstance(a, Out):
                if self.dev:
                    t = torch.full((a.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
                    cargs.append(C.c_void_p(t.data_ptr() + GUARD))
                else:
                    t = np.full(a.nbytes + 2 * GUARD, FILL, np.uint8)
                    cargs.append(C.c_void_p(t.ctypes.data + GUARD))
                outs.append((t, a))
            elif isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                if self.dev and i not in host:
                    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
                    keep.append(t)
                    cargs.append(C.c_void_p(t.data_ptr()))
                else:
                    keep.append(a)
                    cargs.append(a.ctypes.data_as(C.c_void_p))
            else:
                cargs.append(a)
        if self.dev and entry.startswith("dleq"):
            wsb = self.lib.circl_hip_dleq_workspace_size(*counts)
            ws = torch.full((wsb + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")       # (torch's blocks are 256-byte aligned)
            assert GUARD % 8 == 0
            tail = (*counts, C.c_void_p(ws.data_ptr() + GUARD), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        elif self.dev:
            tail = (counts[0], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        else:
            tail = (counts[0], 0)
        self.nat.check(getattr(self.lib, "circl_hip_" + entry + ("_dev" if self.dev else ""))(*cargs, *tail), entry)
        if self.dev and entry.startswith("dleq"):
            torch.cuda.synchronize()
            w = ws.cpu().numpy()
            assert (w[:GUARD] == FILL).all() and (w[GUARD + wsb:] == FILL).all(), entry + ": the workspace's margins"
        res = []
        for t, a in outs:
            if self.dev:
                torch.cuda.synchronize()
                t = t.cpu().numpy()
            assert (t[:GUARD] == FILL).all() and (t[GUARD + a.nbytes:] == FILL).all(), entry
            res.append(t[GUARD:GUARD + a.nbytes].reshape(a.shape).copy())
        return res

    @staticmethod
    def blob(items_):
        if items_ is None:
            return None, None
        off = np.zeros(len(items_) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in items_])
        return np.frombuffer(b"".join(items_) + bytes(16), np.uint8).copy(), off

    @staticmethod
    def _key(x, n):
        """(rows, stride): bytes = one row for the call"""
        return (rows(x), 0) if isinstance(x, bytes) else (rows(x), 32)

    def prove(self, k, kA, B, kB, off, r, ctx, flags=0):
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        dst = np.frombuffer(ctx + b"\0", np.uint8)
        args = [*self._key(k, n), *self._key(kA, n), rows(B), rows(kB), off, rows(r), dst, len(ctx), flags, Out(n, 64), Out(n)]
        return self.run("dleq_prove", args, (n, int(off[-1] - off[0])), host=(8,))

    def verify(self, kA, B, kB, off, proofs, ctx, flags=0):
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        dst = np.frombuffer(ctx + b"\0", np.uint8)
        args = [*self._key(kA, n), rows(B), rows(kB), off, rows(proofs, 64), dst, len(ctx), flags, Out(n)]
        return self.run("dleq_verify", args, (n, int(off[-1] - off[0])), host=(6,))[0]

    def tweak_server(self, sk, infos):
        n = len(infos)
        return self.run("oprf_poprf_tweak", [*self._key(sk, n), None, 0, *self.blob(infos), Out(n, 32), Out(n, 32), Out(n, 32), Out(n)], (n,))

    def tweak_client(self, pk, infos):
        n = len(infos)
        return self.run("oprf_poprf_tweak", [None, 0, *self._key(pk, n), *self.blob(infos), None, None, Out(n, 32), Out(n)], (n,))

    def poprf_finalize(self, inputs, infos, blinds, evaluated):
        n = len(inputs)
        return self.run("oprf_poprf_finalize", [*self.blob(inputs), *self.blob(infos), rows(blinds), rows(evaluated), Out(n, 64), Out(n)], (n,))

    def poprf_full_evaluate(self, sk, inputs, infos):
        n = len(inputs)
        return self.run("oprf_poprf_full_evaluate", [*self._key(sk, n), *self.blob(inputs), *self.blob(infos), Out(n, 64), Out(n)], (n,))

    def evaluate(self, sk, blinded):
        n = len(rows(blinded))
        return self.run("oprf_evaluate", [*self._key(sk, n), rows(blinded), Out(n, 32), Out(n)], (n,))

    def mult(self, k, elems):
        n = len(rows(elems))
        out, ok = self.run("ristretto255_scalar_mult", [*self._key(k, n), rows(elems), 0, Out(n, 32), Out(n)], (n,))
        assert ok.all()
        return out


@pytest.fixture(scope="module", params=FORMS)
def form(request):
    return Form(request.param)


@pytest.fixture(scope="module")
def host():
    return Form("host")


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    return off


def split(a, off):
    return [[a[j].tobytes() for j in range(int(off[g]), int(off[g + 1]))] for g in range(len(off) - 1)]


def scalars(rng, n):
    return [le(1 + int.from_bytes(rng.bytes(32), "little") % (L - 1)) for _ in range(n)]


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_proofs_in_one_call_per_mode(form):
    for cases in (CASES[:3], CASES[3:]):
        ctx = cases[0][1]
        off = offsets([len(c[4]) for c in cases])
        assert list(np.diff(off.astype(np.int64))) == [1, 1, 2]
        B, kB = [x for c in cases for x in c[4]], [x for c in cases for x in c[5]]
        k, kA, r, want = [c[2] for c in cases], [c[3] for c in cases], [c[6] for c in cases], [c[7] for c in cases]
        proofs, ok = form.prove(k, kA, B, kB, off, r, ctx, 1)
        assert [p.tobytes() for p in proofs] == want and ok.tolist() == [1, 1, 1]
        assert form.verify(kA, B, kB, off, want, ctx, 1).tolist() == [1, 1, 1]
        assert form.verify(kA, B, kB, off, [want[0], flip(want[1], 77), want[2]], ctx, 1).tolist() == [1, 0, 1]


# ---- 2. segment shapes ----------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 61, 1, 63, 64, 65, 1, 1, 128, 300, 3]


@pytest.fixture(scope="module")
def segments(host):
    """690 elements in 12 requests, B_j among 15 multiples of the generator; kB for one key and for a key per request"""
    rng = np.random.default_rng(11)
    off = offsets(SIZES)
    n_el = int(off[-1])
    assert n_el == 690 and len(SIZES) == 12
    B = rows([MULT[1 + (7 * j + j // 15) % 15] for j in range(n_el)])
    keys, r = scalars(rng, len(SIZES)), scalars(rng, len(SIZES))
    per_el = rows([keys[g] for g, n in enumerate(SIZES) for _ in range(n)])
    return dict(off=off, B=B, keys=keys, r=r, kA=[oprf.scalar_mult(k)[0] for k in keys], kB_one=host.mult(keys[0], B), kB_own=host.mult(per_el, B))


@pytest.mark.parametrize("keying", ["one-key", "key-per-request"])
def test_segment_shapes(form, segments, keying):
    s, ctx = segments, b"segment shapes"
    off, B = s["off"], s["B"]
    one = keying == "one-key"
    k, kA, kB = (s["keys"][0], s["kA"][0], s["kB_one"]) if one else (s["keys"], s["kA"], s["kB_own"])
    proofs, ok = form.prove(k, kA, B, kB, off, s["r"], ctx)
    Bs, kBs = split(B, off), split(kB, off)
    for g in range(len(SIZES)):
        want = dleq.prove(k if one else k[g], kA if one else kA[g], Bs[g], kBs[g], s["r"][g], ctx)
        assert (proofs[g].tobytes(), int(ok[g])) == want, (g, SIZES[g])
    assert ok.all()
    assert form.verify(kA, B, kB, off, proofs, ctx).tolist() == [1] * len(SIZES)


# ---- 3. tampering ---------------------------------------------------------------------------------------------------------------
def test_tampering_leaves_the_neighbours_alone(form, host):
    rng = np.random.default_rng(12)
    sizes, ctx = [3, 130, 2], b"tampering"
    off = offsets(sizes)
    B = rows([MULT[1 + (3 * j + j // 15) % 15] for j in range(135)])
    (k,), r = scalars(rng, 1), scalars(rng, 3)
    kA, kB = oprf.scalar_mult(k)[0], host.mult(k, B)
    proofs, ok = form.prove(k, kA, B, kB, off, r, ctx)
    assert ok.all() and form.verify(kA, B, kB, off, proofs, ctx).tolist() == [1, 1, 1]

    def case(kA_=None, kB_=None, B_=None, proof_=None):
        kA_ = [kA, kA_ or kA, kA]
        B_, kB_ = B if B_ is None else B_, kB if kB_ is None else kB_
        pr = proofs.copy()
        if proof_ is not None:
            pr[1] = np.frombuffer(proof_, np.uint8)
        got = form.verify(kA_, B_, kB_, off, pr, ctx).tolist()
        want = dleq.verify(kA_[1], split(B_, off)[1], split(kB_, off)[1], pr[1].tobytes(), ctx)
        assert got == [1, want, 1] and want == 0, got

    for j in (0, 63, 64, 129):                  # a flipped bit in kB: first / last lane of the first wave it touches, first of the next, last
        t = kB.copy()
        t[3 + j, 5] ^= 0x10
        case(kB_=t)
    t, u = kB.copy(), B.copy()                  # two pairs swapped: the index j is bound
    assert B[3 + 5].tobytes() != B[3 + 70].tobytes()
    t[[3 + 5, 3 + 70]], u[[3 + 5, 3 + 70]] = t[[3 + 70, 3 + 5]], u[[3 + 70, 3 + 5]]
    case(kB_=t, B_=u)
    p = proofs[1].tobytes()
    case(proof_=flip(p, 6))                     # c
    case(proof_=flip(p, 256 + 6))               # s
    case(kA_=oprf.scalar_mult(le(int.from_bytes(k, "little") + 1))[0])      # another valid key
    case(kA_=flip(kA))                          # does not decode
    c, s = int.from_bytes(p[:32], "little"), int.from_bytes(p[32:], "little")
    case(proof_=le(c + L) + p[32:])
    case(proof_=p[:32] + le(s + L))


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def closed_form():
    """the proof of 65535 copies of one pair, from M = (sum of d_j mod L) B"""
    ctx, k, r = b"limits", le(0x1234567), le(0x7654321)
    kA, b = oprf.scalar_mult(k)[0], MULT[3]
    kb = oprf.scalar_mult(k, b)[0]
    seed = dleq.seed_of(kA, ctx)
    total = sum(dleq.composite_scalar(seed, j, b, kb, ctx) for j in range(dleq.MAX_BATCH)) % L
    ks, rs = int.from_bytes(k, "little"), int.from_bytes(r, "little")
    m = oprf.mul(total, oprf.decode(b))
    c = dleq.challenge(kA, m, oprf.mul(ks, m), oprf.mul(rs, oprf.GENERATOR), oprf.mul(rs, m), ctx)
    return dict(ctx=ctx, k=k, r=r, kA=kA, b=b, kb=kb, proof=le(c) + le((rs - c * ks) % L))


def test_limits_of_a_request(form, closed_form):
    f = closed_form
    sizes = [2, 65535, 65536, 0, 2]
    off, n_el = offsets(sizes), sum(sizes)
    B, kB = np.tile(rows(f["b"]), (n_el, 1)), np.tile(rows(f["kb"]), (n_el, 1))
    B[1], kB[1] = rows(MULT[5])[0], rows(oprf.scalar_mult(f["k"], MULT[5])[0])[0]           # the first request: two different pairs
    B[-1], kB[-1] = B[1], kB[1]                                                             # and the last
    r = [le(77), f["r"], le(78), le(79), le(80)]
    proofs, ok = form.prove(f["k"], f["kA"], B, kB, off, r, f["ctx"])
    assert ok.tolist() == [1, 1, 0, 0, 1]
    assert proofs[1].tobytes() == f["proof"]
    assert not proofs[2].any() and not proofs[3].any()
    for g in (0, 4):
        Bg, kBg = split(B, off)[g], split(kB, off)[g]
        assert proofs[g].tobytes() == dleq.prove(f["k"], f["kA"], Bg, kBg, r[g], f["ctx"])[0]
    pr = proofs.copy()
    pr[2], pr[3] = proofs[1], proofs[0]     # well-formed proofs: the requests fail for their sizes
    assert form.verify(f["kA"], B, kB, off, pr, f["ctx"]).tolist() == [1, 1, 0, 0, 1]


# ---- 5. masks -------------------------------------------------------------------------------------------------------------------
def test_failure_masks(form, host):
    rng = np.random.default_rng(13)
    ctx = b"masks"
    (k,), good_r = scalars(rng, 1), le(4242)
    kA = oprf.scalar_mult(k)[0]
    pair = lambda j: (MULT[j], oprf.scalar_mult(k, MULT[j])[0])
    base = [pair(1 + j % 15) for j in range(70)]
    bad_mid = list(base)
    bad_mid[35] = (base[35][0], flip(base[35][1]))      # s odd: does not decode
    bad_b = list(base)
    bad_b[69] = (flip(base[69][0]), base[69][1])
    ident = [pair(2), (bytes(32), bytes(32)), pair(3)]
    # (k, kA, r, pairs, flags-independent) -- every bad request between good ones
    reqs = [
        (k, kA, good_r, base[:2]),
        (k, kA, bytes(32), base[:2]), (k, kA, le(L), base[:2]), (k, kA, b"\xff" * 32, base[:2]),
        (bytes(32), kA, good_r, base[:2]), (le(L + 5), kA, good_r, base[:2]),
        (k, kA, good_r, base),
        (k, kA, good_r, bad_mid), (k, kA, good_r, bad_b),
        (k, flip(kA), good_r, base[:3]),
        (k, kA, good_r, ident),
        (k, kA, good_r, base[:2]),
    ]
    off = offsets([len(q[3]) for q in reqs])
    B, kB = [p[0] for q in reqs for p in q[3]], [p[1] for q in reqs for p in q[3]]
    ks, kAs, rs = [q[0] for q in reqs], [q[1] for q in reqs], [q[2] for q in reqs]
    for flags in (0, 1):
        want = [dleq.prove(q[0], q[1], [p[0] for p in q[3]], [p[1] for p in q[3]], q[2], ctx, flags) for q in reqs]
        assert [w[1] for w in want] == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1 - flags, 1]
        proofs, ok = form.prove(ks, kAs, B, kB, off, rs, ctx, flags)
        assert ok.tolist() == [w[1] for w in want]
        assert [p.tobytes() for p in proofs] == [w[0] for w in want]
        # the verifier on the same requests, each with a proof that is good for its elements where one exists
        pr = [w[0] if w[1] else want[0][0] for w in want]
        verdict = form.verify(kAs, B, kB, off, pr, ctx, flags).tolist()
        assert verdict == [dleq.verify(q[1], [p[0] for p in q[3]], [p[1] for p in q[3]], p, ctx, flags) for q, p in zip(reqs, pr)]
        assert verdict == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1 - flags, 1]      # (requests 1 .. 5 are request 0 under a bad k or r: its proof verifies)


# ---- 6. the host pipeline's routes ----------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 requests at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices


@pytest.fixture(scope="module")
def pipe():
    from circl_amd import hostapi as api
    import dleq_worker as dw
    return dw.run(api, 0, N_PIPE)


def _check_pipeline_run(o, base):
    from circl_amd import hostapi as api
    import dleq_worker as dw
    for key in base:
        assert (np.asarray(o[key]) == base[key]).all(), key
    assert o["ok"].all() and o["verdict"].all()
    assert o["verdict_bad"].tolist() == [1 - g % 2 for g in range(N_PIPE)]
    k, kA, B, kB, off, r = dw.inputs(api, N_PIPE)
    Bs, kBs = split(B, off), split(kB, off)
    for g in (0, 255, 256, 299):
        assert o["proofs"][g].tobytes() == dleq.prove(k[g].tobytes(), kA[g].tobytes(), Bs[g], kBs[g], r[g].tobytes(), dw.CTX, 1)[0], g
    # the POPRF items
    for key in ("ok_tw", "ok_tw1", "ok_twc", "ok_pfin", "ok_pfin0", "ok_pfull", "ok_pfull0"):
        assert o[key].all(), key
    assert (o["twc"] == o["tw1"]).all()         # pk + m G = (sk + m) G
    infos, ins = dw.item_inputs(N_PIPE)
    b = lambda a: a.tobytes()
    for g in (0, 99, 100, 199, 200, 255, 256, 299):   # both ends, both sides of the shard boundaries and of the chunk boundary
        assert (b(o["t"][g]), b(o["tinv"][g]), b(o["tw"][g]), 1) == dleq.poprf_tweak_server(b(k[g]), infos[g]), g
        assert (b(o["t1"][g]), b(o["tinv1"][g]), b(o["tw1"][g]), 1) == dleq.poprf_tweak_server(b(k[0]), infos[g]), g
        assert (b(o["twc"][g]), 1) == dleq.poprf_tweak_client(b(kA[0]), infos[g]), g
        assert b(o["pfin"][g]) == dleq.poprf_finalize(ins[g], infos[g], b(r[g]), b(kA[g]))[0], g
        assert b(o["pfin0"][g]) == dleq.poprf_finalize(ins[g], b"", b(r[g]), b(kA[g]))[0], g
        assert b(o["pfull"][g]) == dleq.poprf_full_evaluate(b(k[g]), ins[g], infos[g])[0], g
        assert b(o["pfull0"][g]) == dleq.poprf_full_evaluate(b(k[0]), ins[g], b"")[0], g


def test_pipeline_default_run_takes_the_checks(pipe):
    _check_pipeline_run(pipe, pipe)


@pytest.mark.parametrize("env,device", [({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1),
                                        ({"CIRCL_HIP_ZEROCOPY_KB": "0"}, 0)], ids=["chunks", "chunks-in-shards", "merged-copy"])
def test_pipeline_routes_agree(pipe, tmp_path, env, device):
    dst = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dleq_worker.py"), str(device), str(N_PIPE), dst], check=True,
                   env=e, timeout=300)
    _check_pipeline_run(np.load(dst), pipe)


# ---- 7. the POPRF items ---------------------------------------------------------------------------------------------------------
def test_poprf_items_on_the_fixture(form):
    e = G["rfc9497"][2]
    sk, pk = hx(e["skSm"]), hx(e["pkSm"])
    its = [(hx(v["Info"]),) + it for v in e["vectors"] for it in items(v)]
    assert len(its) == 4
    infos, inputs, blinds = [i[0] for i in its], [i[1] for i in its], [i[2] for i in its]
    t, tinv, tg, ok = form.tweak_server(sk, infos)
    want = [dleq.poprf_tweak_server(sk, info) for info in infos]
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


def test_poprf_failure_masks(form):
    info = b"some info"
    m = dleq.info_scalar(info)
    long_info = np.random.default_rng(6).bytes(65536)
    infos = [info, info, long_info, long_info[:-1], b""]
    sks = [le(5), le(L - m), le(5), le(5), le(5)]
    want = [dleq.poprf_tweak_server(s, i) for s, i in zip(sks, infos)]
    t, tinv, tg, ok = form.tweak_server(sks, infos)
    assert ok.tolist() == [1, 0, 0, 1, 1] == [w[3] for w in want]
    assert [(a.tobytes(), b.tobytes(), c.tobytes()) for a, b, c in zip(t, tinv, tg)] == [w[:3] for w in want]
    minus_mg = oprf.encode(oprf.mul(L - m, oprf.GENERATOR))
    pks = [MULT[4], minus_mg, MULT[4], MULT[4], flip(MULT[4])]
    want = [dleq.poprf_tweak_client(p, i) for p, i in zip(pks, infos)]
    tw, ok = form.tweak_client(pks, infos)
    assert ok.tolist() == [1, 0, 0, 1, 0] == [w[1] for w in want] and [x.tobytes() for x in tw] == [w[0] for w in want]
    inputs = [b"x", b"y", b"z", b"", long_info]
    want = [dleq.poprf_full_evaluate(s, x, i) for s, x, i in zip(sks, inputs, infos)]
    out, ok = form.poprf_full_evaluate(sks, inputs, infos)
    assert ok.tolist() == [1, 0, 0, 1, 0] == [w[1] for w in want] and [x.tobytes() for x in out] == [w[0] for w in want]
    blinds, ev = [le(9)] * 5, [MULT[3], MULT[3], MULT[3], bytes(32), MULT[3]]
    want = [dleq.poprf_finalize(x, i, b, e) for x, i, b, e in zip(inputs, infos, blinds, ev)]
    out, ok = form.poprf_finalize(inputs, infos, blinds, ev)
    assert ok.tolist() == [1, 1, 0, 0, 0] == [w[1] for w in want] and [x.tobytes() for x in out] == [w[0] for w in want]
    out, ok = form.poprf_finalize(inputs[:2], None, blinds[:2], ev[:2])     # no infos: every item's is empty
    assert [(x.tobytes(), 1) for x in out] == [dleq.poprf_finalize(x, b"", b, e) for x, b, e in zip(inputs, blinds, ev)][:2]


# ---- 8. the protocol through the wrappers ---------------------------------------------------------------------------------------
class HostWrappers:
    def __init__(self):
        from circl_amd import hostapi as api
        self.api = api

    def blind(self, mode, inputs, blinds):
        return self.api.oprf_blind(mode, inputs, rows(blinds))

    def evaluate_verifiable(self, mode, sk, blinded, off, r, info):
        return self.api.oprf_evaluate_verifiable(mode, sk, blinded, off, rows(r), info)

    def finalize_verifiable(self, mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info):
        return self.api.oprf_finalize_verifiable(mode, pk, inputs, rows(blinds), blinded, evaluated, off, proofs, info)

    def full_evaluate(self, mode, sk, inputs, info):
        if mode == 1:
            return self.api.oprf_full_evaluate(1, sk, inputs)
        return self.api.oprf_poprf_full_evaluate(sk, inputs, [info] * len(inputs))

    def public_key(self, sk):
        return self.api.ristretto255_scalar_mult(sk, n=1)[0][0].tobytes()


class DeviceWrappers:
    def __init__(self):
        import torch
        from circl_amd import device as dev
        self.torch, self.dev, self.o = torch, dev, dev.OprfDevice()

    def t(self, x, width=32):
        return self.torch.from_numpy(rows(x, width).copy()).cuda()

    def blind(self, mode, inputs, blinds):
        out, ok = self.o.blind(mode, self.dev.Ragged(inputs), self.t(blinds))
        return out.cpu().numpy(), ok.cpu().numpy()

    def evaluate_verifiable(self, mode, sk, blinded, off, r, info):
        return tuple(x.cpu().numpy() for x in self.o.evaluate_verifiable(mode, self.t(sk), self.t(blinded), off, self.t(r), info))

    def finalize_verifiable(self, mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info):
        return tuple(x.cpu().numpy() for x in self.o.finalize_verifiable(mode, self.t(pk), self.dev.Ragged(inputs), self.t(blinds), self.t(blinded),
                                                                         self.t(evaluated), off, self.t(proofs, 64), info))

    def full_evaluate(self, mode, sk, inputs, info):
        n = len(inputs)
        if mode == 1:
            out, ok = self.o.full_evaluate(1, self.t(sk), self.dev.Ragged(inputs), n)
        else:
            out, ok = self.o.poprf_full_evaluate(self.t(sk), self.dev.Ragged(inputs), self.dev.Ragged([info] * n), n)
        return out.cpu().numpy(), ok.cpu().numpy()

    def public_key(self, sk):
        return self.o.scalar_mult(self.t(sk), n=1)[0].cpu().numpy()[0].tobytes()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind", FORMS)
def test_protocol_round_trip(kind, mode):
    w = HostWrappers() if kind == "host" else DeviceWrappers()
    rng = np.random.default_rng(14 + mode)
    sizes, info = [1, 2, 70], b"public info" if mode == 2 else b""
    off, n_el = offsets(sizes), sum(sizes)
    (sk,) = scalars(rng, 1)
    pk = w.public_key(sk)
    assert pk == oprf.scalar_mult(sk)[0]
    inputs, blinds, r = [rng.bytes(j % 9) for j in range(n_el)], scalars(rng, n_el), scalars(rng, 3)
    blinded, ok = w.blind(mode, inputs, blinds)
    assert ok.all()
    evaluated, proofs, ok = w.evaluate_verifiable(mode, sk, blinded, off, r, info)
    assert ok.tolist() == [1, 1, 1]
    out, ok = w.finalize_verifiable(mode, pk, inputs, blinds, blinded, evaluated, off, proofs, info)
    full, full_ok = w.full_evaluate(mode, sk, inputs, info)
    assert ok.tolist() == [1, 1, 1] and full_ok.all() and (out == full).all() and out.any(axis=1).all()
    # the checker on the first request, both ends
    want = oprf.full_evaluate(1, sk, inputs[0]) if mode == 1 else dleq.poprf_full_evaluate(sk, inputs[0], info)
    assert (out[0].tobytes(), 1) == want
    # one evaluated element of the middle request replaced by another valid element
    bad = evaluated.copy()
    bad[2] = evaluated[0]
    out2, ok2 = w.finalize_verifiable(mode, pk, inputs, blinds, blinded, bad, off, proofs, info)
    assert ok2.tolist() == [1, 0, 1]
    assert not out2[1:3].any() and (out2[0] == out[0]).all() and (out2[3:] == out[3:]).all()
