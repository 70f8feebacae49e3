"""GPU tests of the batch P-256 / P-384 groups and base-mode OPRF on them (circl_hip_nistp_*, circl_hip_oprf_nistp_*), both forms of every
entry point and both curves, against the CPU checker tests/oprf_nistp.py and the fixture.  Every output of every call lies between guard
margins that must survive.  The sizes are those at which a lane-per-item kernel can go wrong (a partial last wavefront, a second and a
third workgroup, the block edges of SHA-256 and SHA-384, a chunk edge), not workload sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oprf_nistp as on
from conftest import hx
from test_gpu_oprf import Form as _Form, HostBytes, Out
from test_oracle_oprf_nistp import entries, items

pytestmark = pytest.mark.gpu

CURVES = (256, 384)
FORMS = ["host", "dev"]


def J(xs):
    return b"".join(xs)


class Form(_Form):
    """the C ABI of the P-curve block through ctypes, on host buffers or on device tensors: batch-wise, the arguments of tests/oprf_nistp.py
    as lists / joined rows; outputs between guard margins (test_gpu_oprf.Form.run)"""

    @staticmethod
    def rows(x, width, n=None):
        a = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8).reshape(-1, width)
        assert n is None or len(a) == n
        return a

    def hash_to_group(self, curve, msgs, dst, flags=0):
        c = on.CURVES[curve]
        return self.run("nistp_hash_to_group", curve, *self.blob(msgs), HostBytes(dst), len(dst), flags, Out(len(msgs), c.Ne), n=len(msgs))[0]

    def hash_to_scalar(self, curve, msgs, dst):
        c = on.CURVES[curve]
        return self.run("nistp_hash_to_scalar", curve, *self.blob(msgs), HostBytes(dst), len(dst), Out(len(msgs), c.Ns), n=len(msgs))[0]

    def scalar_mult(self, curve, scalars, elems=None, flags=0, n=None, stride=None):
        c = on.CURVES[curve]
        n = n if n is not None else len(self.rows(elems, c.Ne)) if elems is not None else len(self.rows(scalars, c.Ns))
        return self.run("nistp_scalar_mult", curve, self.rows(scalars, c.Ns), c.Ns if stride is None else stride,
                        None if elems is None else self.rows(elems, c.Ne, n), flags, Out(n, c.Ne), Out(n), n=n)

    def derive_keypair(self, curve, mode, seeds, infos):
        c, n = on.CURVES[curve], len(infos)
        return self.run("oprf_nistp_derive_keypair", curve, mode, self.rows(seeds, 32, n), *self.blob(infos), Out(n, c.Ns), Out(n, c.Ne), Out(n), n=n)

    def blind(self, curve, mode, inputs, blinds):
        c, n = on.CURVES[curve], len(inputs)
        return self.run("oprf_nistp_blind", curve, mode, *self.blob(inputs), self.rows(blinds, c.Ns, n), Out(n, c.Ne), Out(n), n=n)

    def evaluate(self, curve, sk, blinded, stride=None):
        c = on.CURVES[curve]
        n = len(self.rows(blinded, c.Ne))
        return self.run("oprf_nistp_evaluate", curve, self.rows(sk, c.Ns), c.Ns if stride is None else stride, self.rows(blinded, c.Ne), Out(n, c.Ne), Out(n), n=n)

    def finalize(self, curve, inputs, blinds, evaluated):
        c, n = on.CURVES[curve], len(inputs)
        return self.run("oprf_nistp_finalize", curve, *self.blob(inputs), self.rows(blinds, c.Ns, n), self.rows(evaluated, c.Ne, n), Out(n, c.Nh), Out(n), n=n)

    def full_evaluate(self, curve, mode, sk, inputs, stride=None):
        c, n = on.CURVES[curve], len(inputs)
        return self.run("oprf_nistp_full_evaluate", curve, mode, self.rows(sk, c.Ns), c.Ns if stride is None else stride, *self.blob(inputs), Out(n, c.Nh),
                        Out(n), n=n)


@pytest.fixture(scope="module", params=FORMS)
def form(request):
    return Form(request.param)


class OneItem:
    """a Form with the per-item signatures of tests/oprf_nistp.py (batches of one)"""

    def __init__(self, form):
        self.f = form

    @staticmethod
    def _t(res):
        return tuple(r[0].tobytes() if r.ndim == 2 else int(r[0]) for r in res)

    def hash_to_group(self, curve, msg, dst, flags=0):
        return self.f.hash_to_group(curve, [msg], dst, flags)[0].tobytes()

    def hash_to_scalar(self, curve, msg, dst):
        return self.f.hash_to_scalar(curve, [msg], dst)[0].tobytes()

    def scalar_mult(self, curve, scalar, elem=None, flags=0):
        return self._t(self.f.scalar_mult(curve, scalar, elem, flags))

    def derive_keypair(self, curve, mode, seed, info):
        return self._t(self.f.derive_keypair(curve, mode, seed, [info]))

    def blind(self, curve, mode, inp, bl):
        return self._t(self.f.blind(curve, mode, [inp], bl))

    def evaluate(self, curve, sk, blinded):
        return self._t(self.f.evaluate(curve, sk, blinded))

    def finalize(self, curve, inp, bl, evaluated):
        return self._t(self.f.finalize(curve, [inp], bl, evaluated))

    def full_evaluate(self, curve, mode, sk, inp):
        return self._t(self.f.full_evaluate(curve, mode, sk, [inp]))


@pytest.mark.parametrize("curve", CURVES)
def test_fixture_vectors(form, curve):
    from test_oprf_nistp_hostsim import check_fixture
    check_fixture(OneItem(form), curve)


# ---- ragged batches against the checker ---------------------------------------------------------------------------------------
LENGTHS = [0, 1, 19, 20, 51, 52, 83, 84, 200]    # around the block edges of the xmd's and the Finalize message's last block for both hashes
DST = b"test_gpu_oprf_nistp"
_REF = {}


def scalar_below_order(c, rng):
    return c.sc(1 + int.from_bytes(rng.bytes(c.Ns), "big") % (c.n - 1))


def ragged_case(curve, n):
    """the inputs of a batch of n and what the checker makes of them, computed once for both forms"""
    if (curve, n) in _REF:
        return _REF[curve, n]
    cv = on.CURVES[curve]
    rng = np.random.default_rng(n + curve)
    lens = [LENGTHS[(i + n) % len(LENGTHS)] for i in range(n)]
    c = dict(n=n, lens=lens, mode=n % 2)
    c["inputs"] = [rng.bytes(k) for k in lens]
    c["infos"] = [rng.bytes((7 * i) % 50) for i in range(n)]
    c["seeds"] = [rng.bytes(32) for _ in range(n)]
    c["blinds"] = [scalar_below_order(cv, rng) for _ in range(n)]
    c["keys"] = [scalar_below_order(cv, rng) for _ in range(n)]
    m = c["mode"]
    ref = {}
    ref["derive"] = [on.derive_keypair(curve, 2 - m, s, i) for s, i in zip(c["seeds"], c["infos"])]
    ref["blind"] = [on.blind(curve, m, x, b) for x, b in zip(c["inputs"], c["blinds"])]
    c["blinded"] = [r[0] for r in ref["blind"]]
    ref["evaluate"] = [on.evaluate(curve, k, e) for k, e in zip(c["keys"], c["blinded"])]
    ref["finalize"] = [on.finalize(curve, x, b, e[0]) for x, b, e in zip(c["inputs"], c["blinds"], ref["evaluate"])]
    ref["full"] = [on.full_evaluate(curve, m, k, x) for k, x in zip(c["keys"], c["inputs"])]
    c["ref"] = ref
    _REF[curve, n] = c
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
@pytest.mark.parametrize("curve", CURVES)
def test_ragged_batch_against_the_checker(form, curve, n):
    """a partial wavefront, exactly one, one and a lane, and a partial third"""
    c = ragged_case(curve, n)
    m, ref = c["mode"], c["ref"]
    same(form.derive_keypair(curve, 2 - m, J(c["seeds"]), c["infos"]), ref["derive"])
    same(form.blind(curve, m, c["inputs"], J(c["blinds"])), ref["blind"])
    same(form.evaluate(curve, J(c["keys"]), J(c["blinded"])), ref["evaluate"])
    same(form.finalize(curve, c["inputs"], J(c["blinds"]), J(e[0] for e in ref["evaluate"])), ref["finalize"])
    same(form.full_evaluate(curve, m, J(c["keys"]), c["inputs"]), ref["full"])


@pytest.mark.parametrize("dst_len", [1, 31, 255])
@pytest.mark.parametrize("curve", CURVES)
def test_hashes_at_every_message_length(form, curve, dst_len):
    """lengths 0..140 in one batch of 141: across the 64- and 128-byte block boundaries of both hashes with the xmd prefix and suffix in place"""
    rng = np.random.default_rng(dst_len + curve)
    dst = rng.bytes(dst_len)
    msgs = [rng.bytes(k) for k in range(141)]
    assert [r.tobytes() for r in form.hash_to_group(curve, msgs, dst)] == [on.hash_to_group(curve, m, dst) for m in msgs]
    assert [r.tobytes() for r in form.hash_to_group(curve, msgs, dst, 1)] == [on.hash_to_group(curve, m, dst, 1) for m in msgs]
    assert [r.tobytes() for r in form.hash_to_scalar(curve, msgs, dst)] == [on.hash_to_scalar(curve, m, dst) for m in msgs]


def bad_encodings(c):
    from test_oprf_nistp_hostsim import bad_encodings as be
    return be(c)


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_mult(form, curve):
    c = on.CURVES[curve]
    rng = np.random.default_rng(31 + curve)
    good = [0, 1, 2, c.n - 1, c.n - 2, (c.n + 1) // 2] + [int.from_bytes(rng.bytes(c.Ns), "big") % c.n for _ in range(4)]
    bad = [c.n, c.n + 1, 2 ** c.bits - 1]
    scalars = [k.to_bytes(c.Ns, "big") for k in good + bad]
    n = len(scalars)
    p = on.hash_to_group(curve, b"a point", DST)
    for flags in (0, 1):        # the generator path and an element, plain and by the inverse (item 0: an inverse of zero)
        want = [on.scalar_mult(curve, s, None, flags) for s in scalars]
        assert [w[1] for w in want] == [1 - flags] + [1] * (len(good) - 1) + [0] * len(bad)
        same(form.scalar_mult(curve, J(scalars), None, flags), want)
        same(form.scalar_mult(curve, J(scalars), p * n, flags), [on.scalar_mult(curve, s, p, flags) for s in scalars])
    # stride 0: one scalar for a batch of 70 elements, among them the identity (in and out with ok = 1) and every undecodable encoding
    elems = [on.hash_to_group(curve, bytes([i]), DST) for i in range(70)]
    undecodable = dict(zip((3, 17, 40, 62, 63, 64, 65, 69), bad_encodings(c)))
    for i, e in undecodable.items():
        elems[i] = e
    elems[5] = bytes(c.Ne)
    k = scalars[7]
    want = [on.scalar_mult(curve, k, e) for e in elems]
    assert [i for i, w in enumerate(want) if not w[1]] == sorted(undecodable) and want[5] == (bytes(c.Ne), 1)
    shared = form.scalar_mult(curve, k, J(elems), stride=0)
    own = form.scalar_mult(curve, k * 70, J(elems))
    same(shared, want)                      # a refused item is a zero row, and its neighbours in the same wavefront are untouched
    same(own, want)
    same(form.scalar_mult(curve, k, None, n=70, stride=0), [on.scalar_mult(curve, k)] * 70)
    same(form.scalar_mult(curve, c.sc(0), J(elems[:3]), stride=0), [(bytes(c.Ne), 1)] * 3)     # identity out


@pytest.mark.parametrize("shared_key", [True, False], ids=["one-key", "key-per-item"])
@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(form, curve, shared_key):
    """finalize(blind(x), evaluate) = full_evaluate(x) = the checker, n = 130 with inputs of 0..129 bytes"""
    c, n = on.CURVES[curve], 130
    rng = np.random.default_rng(130 + curve)
    inputs = [rng.bytes(i) for i in range(n)]
    blinds = [scalar_below_order(c, rng) for _ in range(n)]
    keys = [scalar_below_order(c, rng) for _ in range(n)]
    if shared_key:
        keys = [keys[0]] * n
    sk, stride = (keys[0], 0) if shared_key else (J(keys), None)
    blinded, ok_b = form.blind(curve, 0, inputs, J(blinds))
    evaluated, ok_e = form.evaluate(curve, sk, blinded, stride=stride)
    out, ok_f = form.finalize(curve, inputs, J(blinds), evaluated)
    full, ok_full = form.full_evaluate(curve, 0, sk, inputs, stride=stride)
    assert ok_b.all() and ok_e.all() and ok_f.all() and ok_full.all()
    assert (out == full).all()
    assert [r.tobytes() for r in full] == [on.full_evaluate(curve, 0, k, x)[0] for k, x in zip(keys, inputs)]


@pytest.mark.parametrize("curve", CURVES)
def test_failure_masks(form, curve):
    """zero blind, blind >= n, zero key, identity element, undecodable elements, a 65536-byte input: good items interleaved in the same wavefront"""
    c, n = on.CURVES[curve], 70
    rng = np.random.default_rng(70 + curve)
    inputs = [rng.bytes(i % 23) for i in range(n)]
    inputs[20], inputs[21] = rng.bytes(65536), rng.bytes(65535)
    blinds, keys = [scalar_below_order(c, rng) for _ in range(n)], [scalar_below_order(c, rng) for _ in range(n)]
    elems = [on.hash_to_group(curve, bytes([i]), DST) for i in range(n)]
    bad_elems = dict(zip(range(3, 11), bad_encodings(c)))
    bad_elems[35] = bytes(c.Ne)                                                   # the identity
    for i, e in bad_elems.items():
        elems[i] = e
    bad_scalars = {40: bytes(c.Ns), 41: c.n.to_bytes(c.Ns, "big"), 64: (c.n + 1).to_bytes(c.Ns, "big"), 66: b"\xff" * c.Ns}
    for i, s in bad_scalars.items():
        blinds[i], keys[i] = s, s
    too_long = {20}
    checks = (("evaluate", form.evaluate(curve, J(keys), J(elems)), [on.evaluate(curve, k, e) for k, e in zip(keys, elems)], set(bad_elems) | set(bad_scalars)),
              ("finalize", form.finalize(curve, inputs, J(blinds), J(elems)), [on.finalize(curve, x, b, e) for x, b, e in zip(inputs, blinds, elems)],
               set(bad_elems) | set(bad_scalars) | too_long),
              ("blind", form.blind(curve, 0, inputs, J(blinds)), [on.blind(curve, 0, x, b) for x, b in zip(inputs, blinds)], set(bad_scalars) | too_long),
              ("full_evaluate", form.full_evaluate(curve, 0, J(keys), inputs), [on.full_evaluate(curve, 0, k, x) for k, x in zip(keys, inputs)],
               set(bad_scalars) | too_long),
              ("derive_keypair", form.derive_keypair(curve, 0, bytes(32 * n), inputs), [on.derive_keypair(curve, 0, bytes(32), x) for x in inputs], too_long))
    for name, res, want, bad in checks:
        ok = res[-1]
        assert [i for i in range(n) if not ok[i]] == sorted(bad), name
        assert all(not r[i].any() for r in res[:-1] for i in bad), name
        same(res, want)                                                             # the neighbours are intact


# ---- the wrappers and the host pipeline over a chunk boundary -----------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_wrappers_agree(curve):
    """hostapi.NistpOprf and device.NistpOprfDevice on one small ragged batch, against each other and the checker"""
    import torch
    from circl_amd import device as dv
    from circl_amd import hostapi as api
    c = ragged_case(curve, 65)
    cv, n = on.CURVES[curve], 65
    g, d = api.NistpOprf(curve), dv.NistpOprfDevice(curve)
    t = lambda b, w: torch.from_numpy(np.frombuffer(b, np.uint8).reshape(-1, w).copy()).cuda()
    key, blinds = c["keys"][0], J(c["blinds"])
    rag = dv.Ragged(c["inputs"])
    blinded, _ = g.blind(0, c["inputs"], blinds)
    evaluated, _ = g.evaluate(key, blinded)
    out, ok = g.finalize(c["inputs"], blinds, evaluated)
    full, _ = g.full_evaluate(0, key, c["inputs"])
    d_blinded, _ = d.blind(0, rag, t(blinds, cv.Ns))
    d_eval, _ = d.evaluate(t(key, cv.Ns), d_blinded)
    d_out, d_ok = d.finalize(rag, t(blinds, cv.Ns), d_eval)
    d_full, _ = d.full_evaluate(0, t(key, cv.Ns), rag, n)
    sk, pk, _ = g.derive_keypair(1, J(c["seeds"]), c["infos"])
    d_sk, d_pk, _ = d.derive_keypair(1, t(J(c["seeds"]), 32), dv.Ragged(c["infos"]))
    torch.cuda.synchronize()
    assert ok.all() and d_ok.cpu().numpy().all() and (out == full).all()
    assert (d_out.cpu().numpy() == out).all() and (d_full.cpu().numpy() == full).all()
    assert out[7].tobytes() == on.full_evaluate(curve, 0, key, c["inputs"][7])[0]
    assert (d_sk.cpu().numpy() == sk).all() and (d_pk.cpu().numpy() == pk).all()
    assert (g.scalar_mult(sk)[0] == pk).all() and (d.scalar_mult(d_sk)[0].cpu().numpy() == pk).all()
    assert (d.hash_to_group(rag, n, DST, nonuniform=True).cpu().numpy() == g.hash_to_group(c["inputs"], DST, nonuniform=True)).all()
    assert (d.hash_to_scalar(rag, n, DST).cpu().numpy() == g.hash_to_scalar(c["inputs"], DST)).all()
    assert g.hash_to_scalar(c["inputs"], DST)[3].tobytes() == on.hash_to_scalar(curve, c["inputs"][3], DST)


# run_pipeline splits a shard into chunks of 2^CIRCL_HIP_HOST_CHUNK items, and 8 is the smallest exponent it takes (host_runtime.hip
# host_chunk_items; api_nistp.hip asks for 2^16 by default): 257 is the smallest n that splits, into 256 + 1.
N_PIPE = 257


@pytest.mark.parametrize("curve", CURVES)
def test_host_forms_over_a_chunk_boundary(tmp_path, curve):
    from circl_amd import hostapi as api
    import oprf_nistp_worker as ow
    base = ow.run(api, curve, 0, N_PIPE)
    dst = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e["CIRCL_HIP_HOST_CHUNK"] = "8"
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "oprf_nistp_worker.py"), str(curve), "0", str(N_PIPE), dst],
                   check=True, env=e, timeout=300)
    o = np.load(dst)
    for k in base:
        assert (np.asarray(o[k]) == base[k]).all(), k
    for k in ("ok_keys", "ok_blind", "ok_eval", "ok_eval_own", "ok_fin", "ok_full", "ok_mult", "ok_base"):
        assert o[k].all(), k
    assert (o["output"] == o["full"]).all() and (o["pk_again"] == o["pk"]).all()
    seeds, infos, ins, blinds = ow.inputs(curve, N_PIPE)
    key = o["sk"][0].tobytes()
    for i in (0, 255, 256):
        b = blinds[i].tobytes()
        assert (o["sk"][i].tobytes(), o["pk"][i].tobytes(), 1) == on.derive_keypair(curve, ow.MODE, seeds[i].tobytes(), infos[i])
        assert o["blinded"][i].tobytes() == on.blind(curve, ow.MODE, ins[i], b)[0]
        assert o["evaluated"][i].tobytes() == on.evaluate(curve, key, o["blinded"][i].tobytes())[0]
        assert o["evaluated_own"][i].tobytes() == on.evaluate(curve, o["sk"][i].tobytes(), o["blinded"][i].tobytes())[0]
        assert o["output"][i].tobytes() == on.finalize(curve, ins[i], b, o["evaluated"][i].tobytes())[0]
        assert o["full"][i].tobytes() == on.full_evaluate(curve, ow.MODE, key, ins[i])[0]
        assert o["h2g"][i].tobytes() == on.hash_to_group(curve, ins[i], ow.DST) and o["h2s"][i].tobytes() == on.hash_to_scalar(curve, ins[i], ow.DST)
        assert o["h2g_nu"][i].tobytes() == on.hash_to_group(curve, ins[i], ow.DST, 1)
        assert o["unblinded"][i].tobytes() == on.hash_to_group(curve, ins[i], b"HashToGroup-" + on.CURVES[curve].context_string(ow.MODE))
