"""The HIP kernels on inputs random material almost never produces, byte for byte against the oracle (no tolerances):
sampler paths chosen through tests/golden/rare_paths.json.gz (a third SHAKE256 block for an eta = 4 secret polynomial, the block-1
boundary at eta = 2, a fourth SHAKE128 block for a matrix entry at every position), encapsulation keys with a saturated t^, and the
ring-primitive entry points on inputs at the ends of what they accept.  Those entry points normalise their input to [0, q) before the
transform (prim_kernels.h), so the last group reaches the normalisation and the transforms on 0 and q - 1 in every slot, not the
transforms' lazy ranges: inside the kernels those are reached only through the saturated keys above.
tests/test_oracle_rare_paths.py proves the fixture's claims and checks the oracle on the saturated inputs against plain integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kem_rare_worker
import rare_inputs as ri
from conftest import hx, load_golden
from circl_amd import hostapi
from oracle import orc
from test_gpu_round3 import KEM_ROUTE_IDS, KEM_ROUTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = load_golden("rare_paths.json.gz")
KQ, DQ = 3329, 8380417


# ---- ML-DSA key generation from seeds that leave the samplers' usual path ----------------------------------------------------------------
def _check_keys(param, seeds, special, sign=True):
    n = len(seeds)
    pk, sk = hostapi.mldsa_keygen(param, seeds)
    pk0, sk0 = orc.mldsa_keygen(param, seeds)
    assert (pk == pk0).all() and (sk == sk0).all(), (param, n)
    assert (hostapi.mldsa_public_from_private(param, sk) == pk0).all(), (param, n)      # the decode of the packed s1, s2 in place of the sampler
    if not sign:
        return
    msgs = [b"rare %d" % i for i in range(n)]
    sig = hostapi.mldsa_sign(param, sk, msgs)                                       # with the GPU-made sk
    assert (sig == orc.mldsa_sign(param, sk0, msgs)).all(), (param, n)
    assert hostapi.mldsa_verify(param, pk, sig, msgs).all() and orc.mldsa_verify(param, pk0, sig, msgs).all()
    five = [b"one key %d" % j for j in range(5)]
    for i in special[:2]:
        one = hostapi.mldsa_sign_shared(param, sk[i], five)
        assert (one == orc.mldsa_sign(param, np.tile(sk0[i], (5, 1)), five)).all(), (param, n, i)
        assert hostapi.mldsa_verify_shared(param, pk[i:i + 1], one, five).all()


@pytest.mark.parametrize("param", [65, 3, 44, 87])
def test_mldsa_keygen_on_rare_sampler_seeds(param):
    # 65 / 3: a secret polynomial needs a third SHAKE256 block; 44 / 87: one finishes inside block 1 or on its last nibbles.  Alone, and
    # at both ends of a wavefront's items and of a batch of 70 among ordinary seeds (the last one shares its wavefront with finished lanes)
    for xi in ri.dsa_rare_seeds(FIX, param):
        _check_keys(param, np.frombuffer(xi, np.uint8).reshape(1, 32), [0])
    for seeds, put in ri.dsa_mixed_batches(FIX, param):
        _check_keys(param, seeds, [p for p, _ in put][::-1], sign=len(seeds) == 70)


# ---- ML-KEM / Kyber: fourth-block streams and saturated keys, default routes here, every other route in a process of its own -----------------
@pytest.mark.parametrize("param", [512, 768, 1024])
def test_kem_fourth_block_keys(param):
    assert kem_rare_worker.fourth_block(param) == 6


@pytest.mark.parametrize("param", [512, 768, 1024])
def test_kem_saturated_encapsulation_keys(param):
    assert kem_rare_worker.saturated_keys(param) == 8


@pytest.mark.parametrize("env_extra", KEM_ROUTES[1:], ids=KEM_ROUTE_IDS[1:])
@pytest.mark.parametrize("param", [512, 768, 1024])
def test_kem_rare_inputs_on_every_route(env_extra, param):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kem_rare_worker.py"), str(param)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "kem rare ok %d 6 8" % param in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]


# ---- the ring primitives at the ends of their input ranges, in every exchange form ---------------------------------------------------------
@pytest.fixture(params=[0, 1, 2, 3], ids=["lds", "lds_nowait", "lanes", "lanes_top"])
def form(request, monkeypatch):
    monkeypatch.setenv("CIRCL_HIP_NTT_XCH", str(request.param))   # read at every call (tests/test_gpu_relayout.py)
    return request.param


def _kyber_extremes():
    rows = [np.full(256, KQ - 1), np.full(256, -(KQ - 1)), np.full(256, 32767), np.full(256, -32767),
            np.where(np.arange(256) % 2 == 0, 32767, -32767), np.where(np.arange(256) % 2 == 0, -32767, 32767),
            np.where(np.arange(256) % 2 == 0, KQ - 1, 0), np.where(np.arange(256) % 2 == 0, 0, KQ - 1)]
    return np.concatenate([np.array(rows), np.eye(256, dtype=np.int64) * (KQ - 1)]).astype(np.int16)


def _kyber_in_range(x):
    """the oracle's transforms take coefficients of absolute value below q (pke/kyber/internal/common/ntt.go:54, :141; beyond it their int16 sums wrap), the entry
    points normalise what they are given: larger inputs reach the oracle through ITS normalisation, checked here against x mod q"""
    if np.abs(x.astype(np.int64)).max() < KQ:
        return x
    n = orc.kyber_normalize(x)
    assert (n == x.astype(np.int64) % KQ).all()
    return n


KYBER_WANT = {}


def _kyber_want(kind):
    if not KYBER_WANT:
        p = _kyber_extremes()
        KYBER_WANT["fwd"] = np.stack([orc.kyber_normalize(orc.kyber_ntt(_kyber_in_range(x))) for x in p])
        KYBER_WANT["inv"] = np.stack([orc.kyber_normalize(orc.kyber_invntt(orc.kyber_normalize(x))) for x in p])
        q = np.roll(p, 3, axis=0)                                               # every pattern against another one, and against itself
        KYBER_WANT["mul"] = np.stack([orc.kyber_normalize(orc.kyber_mulhat(orc.kyber_normalize(a), orc.kyber_normalize(b))) for a, b in zip(p, q)])
        KYBER_WANT["sqr"] = np.stack([orc.kyber_normalize(orc.kyber_mulhat(orc.kyber_normalize(a), orc.kyber_normalize(a))) for a in p])
    return KYBER_WANT[kind]


def test_kyber_transforms_at_the_ends_of_the_range(form):
    p = _kyber_extremes()
    for kind, got in (("fwd", hostapi.kyber_ntt(p)), ("inv", hostapi.kyber_ntt(p, inverse=True))):
        bad = np.argwhere(got != _kyber_want(kind))
        assert bad.size == 0, (kind, form, bad[:8].tolist())


def test_kyber_mulhat_at_the_ends_of_the_range():
    # (circl_hip_kyber_mulhat has no exchange and does not read CIRCL_HIP_NTT_XCH: once)
    p = _kyber_extremes()
    for kind, got in (("mul", hostapi.kyber_mulhat(p, np.roll(p, 3, axis=0))), ("sqr", hostapi.kyber_mulhat(p, p))):
        bad = np.argwhere(got != _kyber_want(kind))
        assert bad.size == 0, (kind, bad[:8].tolist())


def _dilithium_extremes():
    rows = [np.full(256, DQ - 1), np.full(256, (1 << 32) - 1), np.full(256, 2 * DQ - 1)]
    return np.concatenate([np.array(rows), np.eye(256, dtype=np.int64) * (DQ - 1)]).astype(np.uint32)


DIL_WANT = {}


def _dilithium_want(kind):
    if not DIL_WANT:
        def ranged(x):   # the oracle's transforms take coefficients below 2q (sign/internal/dilithium/ntt.go:108-110, :188-190): 2^32 - 1 goes through its normalisation
            if int(x.max()) < 2 * DQ:
                return x
            n = orc.dilithium_normalize(x)
            assert (n == x.astype(np.uint64) % DQ).all()
            return n
        p = _dilithium_extremes()
        DIL_WANT["fwd"] = np.stack([orc.dilithium_normalize(orc.dilithium_ntt(ranged(x))) for x in p])
        DIL_WANT["inv"] = np.stack([orc.dilithium_normalize(orc.dilithium_invntt(ranged(x))) for x in p])
    return DIL_WANT[kind]


def test_dilithium_transforms_at_the_ends_of_the_range():
    # (circl_hip_dilithium_ntt has one exchange form and does not read CIRCL_HIP_NTT_XCH: once)
    p = _dilithium_extremes()
    for kind, got in (("fwd", hostapi.dilithium_ntt(p)), ("inv", hostapi.dilithium_ntt(p, inverse=True))):
        bad = np.argwhere(got != _dilithium_want(kind))
        assert bad.size == 0, (kind, bad[:8].tolist())
