"""Batch Ed448-Dilithium3 (sign/eddilithium3) on the GPU: key generation, signing and verification against the oracle's
round-3 Dilithium3 (mode3) and the RFC 8032 5.2 checker of tests/curve448.py, composed as sign/eddilithium3/eddilithium.go does."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import curve448 as ref

pytestmark = pytest.mark.gpu
DPK, DSK, DSIG = 1952, 4000, 3293
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
    rng = np.random.default_rng(31)
    n = 70
    seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 300, n)]
    pk, sk = api.eddilithium3_keygen(seeds)
    sig = api.eddilithium3_sign(sk, msgs)
    return seeds, msgs, pk, sk, sig


def _check_against_oracle_and_checker(orc, seeds, msgs, pk, sk, sig):
    assert pk.shape == (len(seeds), 2009) and sk.shape == (len(seeds), 4057) and sig.shape == (len(seeds), 3407)
    split = [hashlib.shake_256(bytes(s)).digest(32 + 57) for s in seeds]  # NewKeyFromSeed: 32 bytes for mode3, then 57 for Ed448
    sd = np.frombuffer(b"".join(x[:32] for x in split), np.uint8).reshape(-1, 32).copy()
    dpk, dsk = orc.mldsa_keygen(3, sd)
    assert dpk.shape[1] == DPK and dsk.shape[1] == DSK
    assert (pk[:, :DPK] == dpk).all() and (sk[:, :DSK] == dsk).all()
    for i, x in enumerate(split):
        assert bytes(sk[i, DSK:]) == x[32:]  # the Ed448 SEED, not its expanded key
    for i in range(0, len(seeds), 5):
        assert bytes(pk[i, DPK:]) == ref.public(split[i][32:])
    dsig = orc.mldsa_sign(3, dsk, msgs)
    assert dsig.shape[1] == DSIG and (sig[:, :DSIG] == dsig).all()
    for i in range(0, len(seeds), 7):
        esk = split[i][32:] + bytes(pk[i, DPK:])
        assert bytes(sig[i, DSIG:]) == ref.sign(esk, msgs[i], b"")  # the empty context
    assert orc.mldsa_verify(3, dpk, dsig, msgs).all()


def test_keygen_sign_against_oracle_and_checker(batch, orc, api):
    assert api.EDDILITHIUM3_SIZES == dict(seed=57, pk=2009, sk=4057, sig=3407)
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
    rng = np.random.default_rng(32)
    n = 300
    seeds = np.concatenate([seeds70, rng.integers(0, 256, (n - len(seeds70), 57), dtype=np.uint8)])
    lens = rng.permutation(n)  # every length 0..299 once
    lens[[3, 255, 256, 299]] = 0  # ... and empty messages on both sides of the chunk boundary
    msgs = [rng.bytes(int(l)) for l in lens]
    pk, sk, sig, ok = _chunked(3, seeds, msgs, tmp_path)
    _check_against_oracle_and_checker(orc, seeds, msgs, pk, sk, sig)
    assert ok.shape == (n,) and ok.all()
    assert (pk[:70] == pk70).all() and (sk[:70] == sk70).all()


@pytest.mark.parametrize("n", [1, 65])
def test_round_trip_at_boundary_sizes(api, n):
    """one row (the pitch arithmetic of the strided copies is degenerate) and a second, nearly empty wavefront"""
    rng = np.random.default_rng(33 + n)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 100, n)]
    pk, sk = api.eddilithium3_keygen(rng.integers(0, 256, (n, 57), dtype=np.uint8))
    sig = api.eddilithium3_sign(sk, msgs)
    ok = api.eddilithium3_verify(pk, sig, msgs)
    assert ok.shape == (n,) and ok.all()
    for col in (100, DSIG + 70):  # a bit of the Dilithium3 half, a bit of the Ed448 half
        bad = sig.copy()
        bad[:, col] ^= 1
        assert not api.eddilithium3_verify(pk, bad, msgs).any()


def test_verify_both_halves(batch, api):
    seeds, msgs, pk, sk, sig = batch
    assert api.eddilithium3_verify(pk, sig, msgs).all()
    bad = sig.copy()
    bad[0::3, 100] ^= 1         # the Dilithium3 half
    bad[1::3, DSIG + 70] ^= 1   # the Ed448 half (a bit of S)
    ok = api.eddilithium3_verify(pk, bad, msgs)
    assert (ok[0::3] == 0).all() and (ok[1::3] == 0).all() and (ok[2::3] == 1).all()
    bad = sig.copy()
    bad[:, DSIG + 3] ^= 2       # the Ed448 half (a bit of R)
    assert not api.eddilithium3_verify(pk, bad, msgs).any()
    badpk = pk.copy()
    badpk[:, DPK + 3] ^= 8      # the Ed448 half of the key
    assert not api.eddilithium3_verify(badpk, sig, msgs).any()
    badpk = pk.copy()
    badpk[:, 40] ^= 8           # the Dilithium3 half of the key
    assert not api.eddilithium3_verify(badpk, sig, msgs).any()
    other = [m + b"!" for m in msgs]
    assert not api.eddilithium3_verify(pk, sig, other).any()


def test_wrong_lengths_are_false(batch, api):
    seeds, msgs, pk, sk, sig = batch
    sigs = [bytes(sig[0])[:-1], bytes(sig[1]) + b"\0", bytes(sig[2])[:DSIG], bytes(sig[3])]
    pks = [bytes(pk[0]), bytes(pk[1]), bytes(pk[2]), bytes(pk[3])[:DPK]]
    ok = api.eddilithium3_verify(pks, sigs, msgs[:4])
    assert not ok.any()


def test_all_devices(batch, api):
    seeds, msgs, pk, sk, sig = batch
    p2, s2 = api.eddilithium3_keygen(seeds, device=-1)
    assert (p2 == pk).all() and (s2 == sk).all()
    assert (api.eddilithium3_sign(sk, msgs, device=-1) == sig).all()
    assert api.eddilithium3_verify(pk, sig, msgs, device=-1).all()
