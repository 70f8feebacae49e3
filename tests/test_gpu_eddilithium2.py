"""Batch Ed25519-Dilithium2 (sign/eddilithium2) on the GPU: key generation, signing and verification against the oracle's
round-3 Dilithium2 (mode2) and the RFC 8032 checker of tests/ed25519.py, composed as sign/eddilithium2/eddilithium.go does."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ed25519 as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


@pytest.fixture(scope="module")
def batch(api):
    rng = np.random.default_rng(21)
    n = 70
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 300, n)]
    pk, sk = api.eddilithium2_keygen(seeds)
    sig = api.eddilithium2_sign(sk, msgs)
    return seeds, msgs, pk, sk, sig


def _check_against_oracle_and_checker(orc, seeds, msgs, pk, sk, sig):
    assert pk.shape == (len(seeds), 1344) and sk.shape == (len(seeds), 2560) and sig.shape == (len(seeds), 2484)
    split = [hashlib.shake_256(bytes(s)).digest(64) for s in seeds]  # NewKeyFromSeed: 32 bytes for mode2, then 32 for Ed25519
    sd = np.frombuffer(b"".join(x[:32] for x in split), np.uint8).reshape(-1, 32).copy()
    dpk, dsk = orc.mldsa_keygen(2, sd)
    assert (pk[:, :1312] == dpk).all() and (sk[:, :2528] == dsk).all()
    for i, x in enumerate(split):
        assert bytes(sk[i, 2528:]) == x[32:]  # the Ed25519 SEED, not its expanded key
        assert bytes(pk[i, 1312:]) == ref.public(x[32:])
    dsig = orc.mldsa_sign(2, dsk, msgs)
    assert (sig[:, :2420] == dsig).all()
    for i in range(0, len(seeds), 7):
        esk = split[i][32:] + bytes(pk[i, 1312:])
        assert bytes(sig[i, 2420:]) == ref.sign(esk, msgs[i])
    assert orc.mldsa_verify(2, dpk, dsig, msgs).all()


def test_keygen_sign_against_oracle_and_checker(batch, orc):
    _check_against_oracle_and_checker(orc, *batch)


def _chunked(mode, seeds, msgs, tmp_path):
    """keygen, sign and verify in a child process whose pipeline chunks are 2^8 items (the smallest CIRCL_HIP_HOST_CHUNK allows)"""
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    off = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    np.savez(src, seeds=seeds, blob=np.frombuffer(b"".join(msgs), np.uint8), off=off)
    env = dict(os.environ, CIRCL_HIP_HOST_CHUNK="8")
    r = subprocess.run([sys.executable, os.path.join(HERE, "eddilithium_worker.py"), str(mode), src, dst], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = np.load(dst)
    return d["pk"], d["sk"], d["sig"], d["ok"]


def test_second_chunk_of_the_composition(batch, orc, tmp_path):
    """300 items in chunks of 256: the second chunk has rebased message offsets, the workspace of the first and a wipe in between"""
    seeds70, _, pk70, sk70, _ = batch
    rng = np.random.default_rng(22)
    n = 300
    seeds = np.concatenate([seeds70, rng.integers(0, 256, (n - len(seeds70), 32), dtype=np.uint8)])
    lens = rng.permutation(n)  # every length 0..299 once
    lens[[3, 255, 256, 299]] = 0  # ... and empty messages on both sides of the chunk boundary
    msgs = [rng.bytes(int(l)) for l in lens]
    pk, sk, sig, ok = _chunked(2, seeds, msgs, tmp_path)
    _check_against_oracle_and_checker(orc, seeds, msgs, pk, sk, sig)
    assert ok.shape == (n,) and ok.all()
    assert (pk[:70] == pk70).all() and (sk[:70] == sk70).all()


@pytest.mark.parametrize("n", [1, 65])
def test_round_trip_at_boundary_sizes(api, n):
    """one row (the pitch arithmetic of the strided copies is degenerate) and a second, nearly empty wavefront"""
    rng = np.random.default_rng(23 + n)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 100, n)]
    pk, sk = api.eddilithium2_keygen(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    sig = api.eddilithium2_sign(sk, msgs)
    ok = api.eddilithium2_verify(pk, sig, msgs)
    assert ok.shape == (n,) and ok.all()
    for col in (100, 2420 + 40):  # a bit of the Dilithium2 half, a bit of the Ed25519 half
        bad = sig.copy()
        bad[:, col] ^= 1
        assert not api.eddilithium2_verify(pk, bad, msgs).any()


def test_verify_both_halves(batch, api):
    seeds, msgs, pk, sk, sig = batch
    assert api.eddilithium2_verify(pk, sig, msgs).all()
    n = len(msgs)
    bad = sig.copy()
    bad[0::3, 100] ^= 1      # the Dilithium2 half
    bad[1::3, 2420 + 40] ^= 1  # the Ed25519 half (a bit of S)
    ok = api.eddilithium2_verify(pk, bad, msgs)
    assert (ok[0::3] == 0).all() and (ok[1::3] == 0).all() and (ok[2::3] == 1).all()
    badpk = pk.copy()
    badpk[:, 1312 + 3] ^= 8  # the Ed25519 half of the key
    assert not api.eddilithium2_verify(badpk, sig, msgs).any()
    other = [m + b"!" for m in msgs]
    assert not api.eddilithium2_verify(pk, sig, other).any()
    assert n == 70


def test_wrong_lengths_are_false(batch, api):
    seeds, msgs, pk, sk, sig = batch
    sigs = [bytes(sig[0])[:-1], bytes(sig[1]) + b"\0", bytes(sig[2])[:2420], bytes(sig[3])]
    pks = [bytes(pk[0]), bytes(pk[1]), bytes(pk[2]), bytes(pk[3])[:1312]]
    ok = api.eddilithium2_verify(pks, sigs, msgs[:4])
    assert not ok.any()


def test_all_devices(batch, api):
    seeds, msgs, pk, sk, sig = batch
    p2, s2 = api.eddilithium2_keygen(seeds, device=-1)
    assert (p2 == pk).all() and (s2 == sk).all()
    assert (api.eddilithium2_sign(sk, msgs, device=-1) == sig).all()
    assert api.eddilithium2_verify(pk, sig, msgs, device=-1).all()
