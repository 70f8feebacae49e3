"""Batch Ed25519-Dilithium2 (sign/eddilithium2) on the GPU: key generation, signing and verification against the oracle's
round-3 Dilithium2 (mode2) and the RFC 8032 checker of tests/ed25519.py, composed as sign/eddilithium2/eddilithium.go does."""
import hashlib

import numpy as np
import pytest

import ed25519 as ref

pytestmark = pytest.mark.gpu


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


def test_keygen_sign_against_oracle_and_checker(batch, orc):
    seeds, msgs, pk, sk, sig = batch
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
