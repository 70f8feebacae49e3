"""Kyber768-X448 and Kyber1024-X448 (kem/hybrid) on the GPU through the C ABI (circl_hip_hybrid_*, schemes 5 and 6), against the
plain-Python checker of tests/hybrid448.py; the two X448 KeyGen routes (ladder, Ed448 comb) against each other.  The checker's
ladder is slow, so the batches are small and sit on the boundaries: a wavefront and a lane, a second ragged block of the 256-lane
seed-expansion kernel.  The checker's results are computed once per scheme and shared."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import curve448
import hybrid448 as chk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "x448_route_worker.py")
P = curve448.P
X = 56
S5, S6 = chk.KYBER768_X448, chk.KYBER1024_X448


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


class _Reference:
    """the checker's keys, ciphertexts and secrets for the first n items of one scheme's fixed seeds, each item computed once"""

    def __init__(self, scheme):
        self.scheme = scheme
        rng = np.random.default_rng(4480 + scheme)
        self.seeds = rng.integers(0, 256, (257, 64), dtype=np.uint8)
        self.eseeds = rng.integers(0, 256, (257, X), dtype=np.uint8)
        S = chk.sizes(scheme)
        self.pk, self.sk = np.zeros((0, S["pk"]), np.uint8), np.zeros((0, S["sk"]), np.uint8)
        self.ct, self.ss, self.st = np.zeros((0, S["ct"]), np.uint8), np.zeros((0, S["ss"]), np.uint8), np.zeros(0, np.uint8)
        self.ss2 = np.zeros((0, S["ss"]), np.uint8)

    def keys(self, n):
        have = len(self.pk)
        if have < n:
            pk, sk = chk.keygen(self.scheme, self.seeds[have:n])
            self.pk, self.sk = np.concatenate([self.pk, pk]), np.concatenate([self.sk, sk])
        return self.pk[:n].copy(), self.sk[:n].copy()

    def encapsulated(self, n):
        pk, _ = self.keys(n)
        have = len(self.ct)
        if have < n:
            ct, ss, st = chk.encaps(self.scheme, pk[have:n], self.eseeds[have:n])
            self.ct, self.ss, self.st = np.concatenate([self.ct, ct]), np.concatenate([self.ss, ss]), np.concatenate([self.st, st])
        return self.ct[:n].copy(), self.ss[:n].copy(), self.st[:n].copy()

    def decapsulated(self, n):
        _, sk = self.keys(n)
        ct, _, _ = self.encapsulated(n)
        have = len(self.ss2)
        if have < n:
            ss2, st2 = chk.decaps(self.scheme, sk[have:n], ct[have:n])
            assert not st2.any()
            self.ss2 = np.concatenate([self.ss2, ss2])
        return self.ss2[:n].copy()


@pytest.fixture(scope="module")
def refs():
    return {S5: _Reference(S5), S6: _Reference(S6)}


def test_checker_sizes_are_the_abi_sizes(api):
    for s in (S5, S6):
        assert chk.sizes(s) == api.HYBRID_SIZES[s]


# ---- 1: host buffers, a full round trip --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,n", [(S5, 129), (S6, 65)])
def test_host_round_trip_against_the_checker(api, refs, scheme, n):
    R = refs[scheme]
    pk, sk = api.hybrid_keygen(scheme, R.seeds[:n])
    pk0, sk0 = R.keys(n)
    assert (pk == pk0).all() and (sk == sk0).all()
    ct, ss, st = api.hybrid_encaps(scheme, pk, R.eseeds[:n])
    ct0, ss0, st0 = R.encapsulated(n)
    assert not st.any() and not st0.any()
    assert (ct == ct0).all() and (ss == ss0).all()
    ss2, st2 = api.hybrid_decaps(scheme, sk, ct)
    assert not st2.any()
    assert (ss2 == R.decapsulated(n)).all() and (ss2 == ss).all()
    assert ss[:, :X].any(axis=1).all() and ss[:, X:].any(axis=1).all()


# ---- 2: key generation over a ragged second block of the 256-lane expansion kernel -----------------------------------------
def test_keygen_across_launch_blocks(api, refs):
    n = 257
    pk, sk = api.hybrid_keygen(S5, refs[S5].seeds[:n])
    pk0, sk0 = refs[S5].keys(n)
    assert (pk == pk0).all() and (sk == sk0).all()


# ---- 3: the device-resident calls and what they leave in the workspace --------------------------------------------------------
def _up256(x):
    return (x + 255) // 256 * 256


def _regions(order, n):
    """byte ranges of a call's carved temporaries, in the order api_hybrid.hip takes them (each rounded up to 256 bytes)"""
    at, out = 0, {}
    for name, row in order:
        out[name] = (at, at + n * row)
        at += _up256(n * row)
    return out


@pytest.mark.parametrize("scheme", [S5, S6])
def test_device_resident_calls_and_their_wipes(api, refs, scheme):
    import torch
    from circl_amd import device as dv
    n = 65
    R = refs[scheme]
    S = chk.sizes(scheme)
    EK, DK, CT = S["pk"] - X, S["sk"] - X, S["ct"] - X
    H = dv.HybridDevice(scheme, n)
    assert H.S == S
    tmp = H.wsb - H.L.circl_hip_mlkem_workspace_size(chk.PARAM[scheme], n)  # the hybrid's own temporaries sit in front of the Kyber workspace
    assert 0 < tmp < H.wsb
    pk0, sk0 = R.keys(n)
    ct0, ss0, _ = R.encapsulated(n)
    ex = [hashlib.shake_256(bytes(s)).digest(X + 64) for s in R.seeds[:n]]
    eex = [hashlib.shake_256(bytes(s)).digest(X + 32) for s in R.eseeds[:n]]
    ekx = [hashlib.shake_256(e[:X]).digest(X) for e in eex]

    def ws_after():
        torch.cuda.synchronize()
        return H.ws[:tmp].cpu().numpy()

    def absent(blob, secrets):
        raw = blob.tobytes()
        return all(bytes(s) not in raw for s in secrets)

    H.ws.fill_(0x77)
    pk, sk = H.keygen(torch.from_numpy(R.seeds[:n]).cuda())
    assert (pk.cpu().numpy() == pk0).all() and (sk.cpu().numpy() == sk0).all()
    w = ws_after()
    reg = _regions([("seedm", 64), ("skx", X), ("pkx", X), ("ek", EK), ("dk", DK)], n)
    for name in ("seedm", "skx", "dk"):
        assert not w[reg[name][0]:reg[name][1]].any(), name
    assert (w[reg["pkx"][0]:reg["pkx"][1]].reshape(n, X) == pk0[:, :X]).all()  # (the layout above is the call's: the public half is where it says)
    assert absent(w, [r[:X] for r in sk0]) and absent(w, [e[X:] for e in ex]) and absent(w, [r[X:X + 64] for r in sk0])

    H.ws.fill_(0x77)
    ct, ss, st = H.encaps(pk, torch.from_numpy(R.eseeds[:n]).cuda())
    assert not st.cpu().numpy().any()
    assert (ct.cpu().numpy() == ct0).all() and (ss.cpu().numpy() == ss0).all()
    w = ws_after()
    reg = _regions([("ek", EK), ("pkx", X), ("m", 32), ("ekx", X), ("ctm", CT), ("ssm", 32), ("ctx", X), ("ssx", X)], n)
    for name in ("m", "ekx", "ssm", "ssx"):
        assert not w[reg[name][0]:reg[name][1]].any(), name
    assert (w[reg["ctx"][0]:reg["ctx"][1]].reshape(n, X) == ct0[:, :X]).all()
    assert absent(w, ekx) and absent(w, [r[:X] for r in ss0]) and absent(w, [r[X:] for r in ss0]) and absent(w, [e[X:] for e in eex])

    H.ws.fill_(0x77)
    ss2, st2 = H.decaps(sk, ct)
    assert not st2.cpu().numpy().any() and (ss2.cpu().numpy() == ss0).all()
    w = ws_after()
    reg = _regions([("dk", DK), ("ek", EK), ("skx", X), ("ctm", CT), ("ctx", X), ("ssm", 32), ("ssx", X)], n)
    for name in ("dk", "skx", "ssm", "ssx"):
        assert not w[reg[name][0]:reg[name][1]].any(), name
    assert absent(w, [r[:X] for r in sk0]) and absent(w, [r[:X] for r in ss0]) and absent(w, [r[X:] for r in ss0])


# ---- 4: where x448.Shared refuses the point ---------------------------------------------------------------------------------
def _enc(v):
    return np.frombuffer(v.to_bytes(X, "little"), np.uint8)


def test_failing_x448_half(api, refs):
    n = 8
    R = refs[S5]
    pk, sk = R.keys(n)
    patch = {1: 0, 3: 1, 5: P - 1, 6: P + 1, 7: P + 2}  # p + 1 is not canonical and reduces to 1; p + 2 reduces to 2, an ordinary point
    bad = [1, 3, 5, 6]
    for i, v in patch.items():
        pk[i, :X] = _enc(v)
    ct, ss, st = api.hybrid_encaps(S5, pk, R.eseeds[:n])
    ct0, ss0, st0 = chk.encaps(S5, pk, R.eseeds[:n])
    assert [int(x) for x in st] == [1 if i in bad else 0 for i in range(n)] == [int(x) for x in st0]
    assert not ct[bad].any() and not ss[bad].any()
    assert (ct == ct0).all() and (ss == ss0).all()
    good = [i for i in range(n) if i not in bad]
    assert ct[good].any(axis=1).all() and ss[good, :X].any(axis=1).all()
    # the same points as the X448 half of a ciphertext
    ct_ok, _, _ = R.encapsulated(n)
    for i, v in patch.items():
        ct_ok[i, :X] = _enc(v)
    ss2, st2 = api.hybrid_decaps(S5, sk, ct_ok)
    ss20, st20 = chk.decaps(S5, sk, ct_ok)
    assert [int(x) for x in st2] == [1 if i in bad else 0 for i in range(n)] == [int(x) for x in st20]
    assert not ss2[bad].any() and (ss2 == ss20).all() and ss2[good].any(axis=1).all()


# ---- 5: the two KeyGen routes, one fresh process each -------------------------------------------------------------------------
def test_keygen_routes_agree(api, tmp_path):
    import x448_route_worker as worker
    got = {}
    for route in ("ladder", "comb"):  # the second child starts only after the first came back with 0
        out = str(tmp_path / (route + ".npz"))
        r = subprocess.run([sys.executable, WORKER, out], cwd=ROOT, env=dict(os.environ, CIRCL_HIP_X448_KEYGEN=route), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, route + ": " + r.stdout[-2000:] + r.stderr[-4000:]
        got[route] = np.load(out)
        assert str(got[route]["route"]) == route
    a, b = got["ladder"], got["comb"]
    assert a["pub"].shape == (worker.N_KEYGEN, X) and a["ok"].all() and b["ok"].all()
    for f in ("pub", "pk", "ct", "ss", "st"):
        assert (a[f] == b[f]).all(), f
    k, seeds, eseeds = worker.inputs()
    for i in range(32):
        assert bytes(a["pub"][i]) == curve448.x448(bytes(k[i]))[0], i
    # ... and the encapsulation (the pair kernel, by either route) is this process's
    pk, _ = api.hybrid_keygen(S5, seeds)
    ct, ss, st = api.hybrid_encaps(S5, pk, eseeds)
    assert (pk == a["pk"]).all() and (ct == a["ct"]).all() and (ss == a["ss"]).all() and not st.any() and not a["st"].any()


# ---- 6: the pair kernel's base-point half against the single KeyGen launch ------------------------------------------------
def test_pair_kernel_public_half(api, refs):
    n = 65
    R = refs[S5]
    pk, _ = api.hybrid_keygen(S5, R.seeds[:n])
    ct, ss, st = api.hybrid_encaps(S5, pk, R.eseeds[:n])
    assert not st.any()
    ekx = np.stack([np.frombuffer(hashlib.shake_256(hashlib.shake_256(bytes(s)).digest(X)).digest(X), np.uint8) for s in R.eseeds[:n]])
    pub, ok = api.x448(ekx)
    assert ok.all() and (ct[:, :X] == pub).all()
    shared, ok2 = api.x448(ekx, pk[:, :X].copy())
    assert ok2.all() and (ss[:, :X] == shared).all()
