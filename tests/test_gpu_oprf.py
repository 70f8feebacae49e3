"""GPU tests of the batch ristretto255 group and base-mode OPRF (circl_hip_ristretto255_*, circl_hip_oprf_*), both forms of every entry
point, against the CPU checker tests/oprf.py and the fixture.  Every output of every call lies between guard margins that must
survive.  The sizes are those at which a lane-per-item kernel can go wrong (a partial last wavefront, a second workgroup, SHA-512's
padding edges, chunk edges), not workload sizes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oprf
from conftest import hx, load_golden
from test_oracle_oprf import items

pytestmark = pytest.mark.gpu

G = load_golden("oprf_ristretto255.json.gz")
GUARD, FILL = 64, 0xA5
L = oprf.L
FORMS = ["host", "dev"]


def le(x):
    return x.to_bytes(32, "little")


class Out:
    def __init__(self, *shape):
        self.shape = shape
        self.nbytes = int(np.prod(shape))


class HostBytes:
    """an argument that stays in host memory in both forms (the tag of the group-level hashes)"""

    def __init__(self, b):
        self.a = np.frombuffer(bytes(b) + b"\0", np.uint8)


def rows(x, n=None):
    a = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8).reshape(-1, 32)
    assert n is None or len(a) == n
    return a


class Form:
    """the C ABI through ctypes, on host buffers or on device tensors: inputs are numpy arrays, outputs are allocated here between guard
    margins, checked and returned as numpy arrays"""

    def __init__(self, kind):
        from circl_amd import _native as nat
        from circl_amd import build as cbuild
        cbuild.build()
        self.nat, self.lib, self.dev = nat, nat.lib(), kind == "dev"

    def run(self, entry, *args, n):
        import torch
        keep, outs, cargs = [], [], []
        for a in args:
            if isinstance(a, Out):
                if self.dev:
                    t = torch.full((a.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
                    cargs.append(C.c_void_p(t.data_ptr() + GUARD))
                else:
                    t = np.full(a.nbytes + 2 * GUARD, FILL, np.uint8)
                    cargs.append(C.c_void_p(t.ctypes.data + GUARD))
                outs.append((t, a))
            elif isinstance(a, HostBytes):
                keep.append(a)
                cargs.append(a.a.ctypes.data_as(C.c_void_p))
            elif isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                if self.dev:
                    t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
                    keep.append(t)
                    cargs.append(C.c_void_p(t.data_ptr()))
                else:
                    keep.append(a)
                    cargs.append(a.ctypes.data_as(C.c_void_p))
            else:
                cargs.append(a)
        tail = C.c_void_p(torch.cuda.current_stream().cuda_stream) if self.dev else 0
        self.nat.check(getattr(self.lib, "circl_hip_" + entry + ("_dev" if self.dev else ""))(*cargs, n, tail), entry)
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
        off = np.zeros(len(items_) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in items_])
        return np.frombuffer(b"".join(items_) + bytes(16), np.uint8).copy(), off

    # the operations, batch-wise: the arguments of tests/oprf.py as lists / (n, 32) arrays
    def hash_to_group(self, msgs, dst):
        return self.run("ristretto255_hash_to_group", *self.blob(msgs), HostBytes(dst), len(dst), Out(len(msgs), 32), n=len(msgs))[0]

    def hash_to_scalar(self, msgs, dst):
        return self.run("ristretto255_hash_to_scalar", *self.blob(msgs), HostBytes(dst), len(dst), Out(len(msgs), 32), n=len(msgs))[0]

    def scalar_mult(self, scalars, elems=None, flags=0, n=None, stride=32):
        n = n if n is not None else len(rows(elems)) if elems is not None else len(rows(scalars))
        return self.run("ristretto255_scalar_mult", rows(scalars), stride, None if elems is None else rows(elems, n), flags, Out(n, 32), Out(n), n=n)

    def derive_keypair(self, mode, seeds, infos):
        n = len(infos)
        return self.run("oprf_derive_keypair", mode, rows(seeds, n), *self.blob(infos), Out(n, 32), Out(n, 32), Out(n), n=n)

    def blind(self, mode, inputs, blinds):
        n = len(inputs)
        return self.run("oprf_blind", mode, *self.blob(inputs), rows(blinds, n), Out(n, 32), Out(n), n=n)

    def evaluate(self, sk, blinded, stride=32):
        n = len(rows(blinded))
        return self.run("oprf_evaluate", rows(sk), stride, rows(blinded), Out(n, 32), Out(n), n=n)

    def finalize(self, inputs, blinds, evaluated):
        n = len(inputs)
        return self.run("oprf_finalize", *self.blob(inputs), rows(blinds, n), rows(evaluated, n), Out(n, 64), Out(n), n=n)

    def full_evaluate(self, mode, sk, inputs, stride=32):
        n = len(inputs)
        return self.run("oprf_full_evaluate", mode, rows(sk), stride, *self.blob(inputs), Out(n, 64), Out(n), n=n)


@pytest.fixture(scope="module", params=FORMS)
def form(request):
    return Form(request.param)


class OneItem:
    """a Form with the per-item signatures of tests/oprf.py (batches of one)"""

    def __init__(self, form):
        self.f = form

    @staticmethod
    def _t(res):
        return tuple(r[0].tobytes() if r.ndim == 2 else int(r[0]) for r in res)

    def hash_to_group(self, msg, dst):
        return self.f.hash_to_group([msg], dst)[0].tobytes()

    def hash_to_scalar(self, msg, dst):
        return self.f.hash_to_scalar([msg], dst)[0].tobytes()

    def scalar_mult(self, scalar, elem=None, flags=0):
        return self._t(self.f.scalar_mult(scalar, elem, flags))

    def derive_keypair(self, mode, seed, info):
        return self._t(self.f.derive_keypair(mode, seed, [info]))

    def blind(self, mode, inp, bl):
        return self._t(self.f.blind(mode, [inp], bl))

    def evaluate(self, sk, blinded):
        return self._t(self.f.evaluate(sk, blinded))

    def finalize(self, inp, bl, evaluated):
        return self._t(self.f.finalize([inp], bl, evaluated))

    def full_evaluate(self, mode, sk, inp):
        return self._t(self.f.full_evaluate(mode, sk, [inp]))


def test_fixture_vectors(form):
    from test_oprf_hostsim import check_fixture
    check_fixture(OneItem(form))


# ---- ragged batches against the checker ---------------------------------------------------------------------------------------
LENGTHS = [0, 1, 67, 68, 83, 84, 85, 195, 196, 1000]     # 67 | 68 and 83 | 84: the xmd and the Finalize message cross SHA-512's padding edges
DST = b"test_gpu_oprf-ristretto255-SHA512"
_REF = {}


def scalar_below_order(rng):
    return le(1 + int.from_bytes(rng.bytes(32), "little") % (L - 1))


def ragged_case(n):
    """the inputs of a batch of n and what the checker makes of them, computed once for both forms"""
    if n in _REF:
        return _REF[n]
    rng = np.random.default_rng(n)
    lens = [LENGTHS[(i + n) % len(LENGTHS)] for i in range(n)]
    if n >= 63:
        lens[5], lens[61] = 65535, 65536       # the longest input RFC 9497 allows, and one byte more
    c = dict(n=n, lens=lens, mode=n % 2)
    c["inputs"] = [rng.bytes(k) for k in lens]
    c["infos"] = [rng.bytes((7 * i) % 50) for i in range(n)]
    c["seeds"] = [rng.bytes(32) for _ in range(n)]
    c["blinds"] = [scalar_below_order(rng) for _ in range(n)]
    c["keys"] = [scalar_below_order(rng) for _ in range(n)]
    m = c["mode"]
    ref = {}
    ref["derive"] = [oprf.derive_keypair(2 - m, s, i) for s, i in zip(c["seeds"], c["infos"])]
    ref["blind"] = [oprf.blind(m, x, b) for x, b in zip(c["inputs"], c["blinds"])]
    blinded = [r[0] if r[1] else oprf.hash_to_group(b"stand-in", DST) for r in ref["blind"]]      # a failed item still gets a valid element to evaluate
    ref["evaluate"] = [oprf.evaluate(k, e) for k, e in zip(c["keys"], blinded)]
    ref["finalize"] = [oprf.finalize(x, b, e[0]) for x, b, e in zip(c["inputs"], c["blinds"], ref["evaluate"])]
    ref["full"] = [oprf.full_evaluate(m, k, x) for k, x in zip(c["keys"], c["inputs"])]
    ref["h2g"] = [oprf.hash_to_group(x, DST) for x in c["inputs"]]
    ref["h2s"] = [oprf.hash_to_scalar(x, DST) for x in c["inputs"]]
    ref["mult"] = [oprf.scalar_mult(k, e, 1) for k, e in zip(c["keys"], blinded)]
    ref["base"] = [oprf.scalar_mult(k) for k in c["keys"]]
    c["blinded"], c["ref"] = blinded, ref
    _REF[n] = c
    return c


def same(got, want):
    """the arrays a Form returned against the checker's per-item tuples"""
    for j, g in enumerate(got):
        w = [t[j] for t in want]
        if g.ndim == 2:
            assert [r.tobytes() for r in g] == w, j
        else:
            assert g.tolist() == w, j


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ragged_batch_against_the_checker(form, n):
    c = ragged_case(n)
    m, ref = c["mode"], c["ref"]
    if n >= 63:
        assert [ref[k][61][-1] for k in ("blind", "finalize", "full")] == [0, 0, 0] and [ref[k][5][-1] for k in ("blind", "finalize", "full")] == [1, 1, 1]
    J = lambda xs: b"".join(xs)
    same(form.derive_keypair(2 - m, J(c["seeds"]), c["infos"]), ref["derive"])
    same(form.blind(m, c["inputs"], J(c["blinds"])), ref["blind"])
    same(form.evaluate(J(c["keys"]), J(c["blinded"])), ref["evaluate"])
    same(form.finalize(c["inputs"], J(c["blinds"]), J(e[0] for e in ref["evaluate"])), ref["finalize"])
    same(form.full_evaluate(m, J(c["keys"]), c["inputs"]), ref["full"])
    assert [r.tobytes() for r in form.hash_to_group(c["inputs"], DST)] == ref["h2g"]
    assert [r.tobytes() for r in form.hash_to_scalar(c["inputs"], DST)] == ref["h2s"]
    same(form.scalar_mult(J(c["keys"]), J(c["blinded"]), 1), ref["mult"])
    same(form.scalar_mult(J(c["keys"])), ref["base"])


# ---- the wrappers: round trip and shared key ------------------------------------------------------------------------------------
def test_round_trip_through_the_wrappers():
    """finalize(evaluate(blind(x))) = full_evaluate(x) for a whole batch, through hostapi and through device.OprfDevice"""
    import torch
    from circl_amd import device as dv
    from circl_amd import hostapi as api
    c = ragged_case(130)
    key, blinds = c["keys"][0], rows(b"".join(c["blinds"]))
    blinded, ok_b = api.oprf_blind(0, c["inputs"], blinds)
    evaluated, ok_e = api.oprf_evaluate(key, blinded)
    out, ok_f = api.oprf_finalize(c["inputs"], blinds, evaluated)
    full, ok_full = api.oprf_full_evaluate(0, key, c["inputs"])
    want_ok = [int(k <= 65535) for k in c["lens"]]
    assert ok_b.tolist() == want_ok and ok_f.tolist() == want_ok and ok_full.tolist() == want_ok
    assert ok_e.tolist() == want_ok                   # the one refused input left a zero row: the identity, which Evaluate refuses
    assert (out == full).all() and out[0].tobytes() == oprf.full_evaluate(0, key, c["inputs"][0])[0]
    d = dv.OprfDevice()
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
    rag = dv.Ragged(c["inputs"])
    d_blinded, _ = d.blind(0, rag, t(blinds))
    d_eval, _ = d.evaluate(t(rows(key)), d_blinded)
    d_out, d_ok = d.finalize(rag, t(blinds), d_eval)
    d_full, _ = d.full_evaluate(0, t(rows(key)), rag, 130)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == out).all() and (d_full.cpu().numpy() == full).all() and d_ok.cpu().numpy().tolist() == want_ok
    sk, pk, _ = api.oprf_derive_keypair(1, rows(b"".join(c["seeds"])), c["infos"])
    d_sk, d_pk, _ = d.derive_keypair(1, t(rows(b"".join(c["seeds"]))), dv.Ragged(c["infos"]))
    assert (d_sk.cpu().numpy() == sk).all() and (d_pk.cpu().numpy() == pk).all()
    assert (api.ristretto255_scalar_mult(sk)[0] == pk).all() and (d.scalar_mult(d_sk)[0].cpu().numpy() == pk).all()
    assert (d.hash_to_group(rag, 130, DST).cpu().numpy() == api.ristretto255_hash_to_group(c["inputs"], DST)).all()
    assert (d.hash_to_scalar(rag, 130, DST).cpu().numpy() == api.ristretto255_hash_to_scalar(c["inputs"], DST)).all()


def test_shared_key_equals_per_item_keys(form):
    c = ragged_case(65)
    n, key = 65, c["keys"][3]
    blinded = b"".join(c["blinded"])
    for shared, own in ((form.evaluate(key, blinded, stride=0), form.evaluate(key * n, blinded)),
                        (form.full_evaluate(1, key, c["inputs"], stride=0), form.full_evaluate(1, key * n, c["inputs"])),
                        (form.scalar_mult(key, blinded, 1, stride=0), form.scalar_mult(key * n, blinded, 1)),
                        (form.scalar_mult(key, None, 0, n=n, stride=0), form.scalar_mult(key * n))):
        assert (shared[0] == own[0]).all() and (shared[1] == own[1]).all() and shared[1][:5].tolist() == [1] * 5
    assert form.evaluate(key, blinded, stride=0)[0][7].tobytes() == oprf.evaluate(key, c["blinded"][7])[0]


# ---- failure masks, in the middle of a batch of 70 ----------------------------------------------------------------------------
def test_failure_masks(form):
    n = 70
    c = ragged_case(65)
    rng = np.random.default_rng(70)
    inputs = [rng.bytes(i % 23) for i in range(n)]
    blinds, keys = [scalar_below_order(rng) for _ in range(n)], [scalar_below_order(rng) for _ in range(n)]
    elems = [c["blinded"][i % 65] for i in range(n)]
    bad_elems = {3 + j: hx(x["enc"]) for j, x in enumerate(G["invalid"])}      # items 3..31: every invalid encoding of the fixture
    bad_elems[35] = bytes(32)                                                   # the identity
    assert len(bad_elems) == 30
    for i, e in bad_elems.items():
        elems[i] = e
    bad_scalars = {40: bytes(32), 41: le(L), 64: le(L + 1)}                     # 0, L, and one in the second wavefront
    for i, s in bad_scalars.items():
        blinds[i], keys[i] = s, s
    J = lambda xs: b"".join(xs)
    checks = (("evaluate", form.evaluate(J(keys), J(elems)), [oprf.evaluate(k, e) for k, e in zip(keys, elems)], set(bad_elems) | set(bad_scalars)),
              ("finalize", form.finalize(inputs, J(blinds), J(elems)), [oprf.finalize(x, b, e) for x, b, e in zip(inputs, blinds, elems)],
               set(bad_elems) | set(bad_scalars)),
              ("blind", form.blind(0, inputs, J(blinds)), [oprf.blind(0, x, b) for x, b in zip(inputs, blinds)], set(bad_scalars)),
              ("full_evaluate", form.full_evaluate(0, J(keys), inputs), [oprf.full_evaluate(0, k, x) for k, x in zip(keys, inputs)], set(bad_scalars)),
              ("scalar_mult", form.scalar_mult(J(keys), J(elems)), [oprf.scalar_mult(k, e) for k, e in zip(keys, elems)],
               (set(bad_elems) - {35}) | {41, 64}),                            # here the identity and the scalar 0 are accepted
              ("scalar_mult by the inverse", form.scalar_mult(J(keys), J(elems), 1), [oprf.scalar_mult(k, e, 1) for k, e in zip(keys, elems)],
               (set(bad_elems) - {35}) | set(bad_scalars)))
    for name, (out, ok), want, bad in checks:
        assert [i for i in range(n) if not ok[i]] == sorted(bad), name
        assert all(not out[i].any() for i in bad), name
        same((out, ok), want)                                                   # the neighbours are intact


# ---- the host pipeline's routes -------------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 items at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices


@pytest.fixture(scope="module")
def pipe():
    from circl_amd import hostapi as api
    import oprf_worker as ow
    return ow.run(api, 0, N_PIPE)


def _check_pipeline_run(o, base):
    import oprf_worker as ow
    for k in base:
        assert (np.asarray(o[k]) == base[k]).all(), k
    for k in ("ok_keys", "ok_blind", "ok_eval", "ok_eval_own", "ok_fin", "ok_full", "ok_mult", "ok_base"):
        assert o[k].all(), k
    assert (o["output"] == o["full"]).all() and (o["pk_again"] == o["pk"]).all()
    seeds, infos, ins, blinds = ow.inputs(N_PIPE)
    key = o["sk"][0].tobytes()
    for i in (0, 255, 256, 299):
        b = blinds[i].tobytes()
        assert (o["sk"][i].tobytes(), o["pk"][i].tobytes(), 1) == oprf.derive_keypair(ow.MODE, seeds[i].tobytes(), infos[i])
        assert o["blinded"][i].tobytes() == oprf.blind(ow.MODE, ins[i], b)[0]
        assert o["evaluated"][i].tobytes() == oprf.evaluate(key, o["blinded"][i].tobytes())[0]
        assert o["evaluated_own"][i].tobytes() == oprf.evaluate(o["sk"][i].tobytes(), o["blinded"][i].tobytes())[0]
        assert o["output"][i].tobytes() == oprf.finalize(ins[i], b, o["evaluated"][i].tobytes())[0]
        assert o["full"][i].tobytes() == oprf.full_evaluate(ow.MODE, key, ins[i])[0]
        assert o["h2g"][i].tobytes() == oprf.hash_to_group(ins[i], ow.DST) and o["h2s"][i].tobytes() == oprf.hash_to_scalar(ins[i], ow.DST)
        assert o["unblinded"][i].tobytes() == oprf.hash_to_group(ins[i], b"HashToGroup-" + oprf.context_string(ow.MODE))


def test_pipeline_default_run_takes_the_checks(pipe):
    _check_pipeline_run(pipe, pipe)


@pytest.mark.parametrize("env,device", [({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1),
                                        ({"CIRCL_HIP_ZEROCOPY_KB": "0"}, 0)], ids=["chunks", "chunks-in-shards", "merged-copy"])
def test_pipeline_routes_agree(pipe, tmp_path, env, device):
    dst = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oprf_worker.py"), str(device), str(N_PIPE), dst], check=True,
                   env=e, timeout=300)
    _check_pipeline_run(np.load(dst), pipe)
