"""Batch Ed448-Dilithium3 (sign/eddilithium3) on the GPU: key generation, signing and verification against the oracle's
round-3 Dilithium3 (mode3) and the RFC 8032 5.2 checker of tests/curve448.py, composed as sign/eddilithium3/eddilithium.go does."""
import hashlib

import numpy as np
import pytest

import curve448 as ref

pytestmark = pytest.mark.gpu
DPK, DSK, DSIG = 1952, 4000, 3293


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


def test_keygen_sign_against_oracle_and_checker(batch, orc, api):
    seeds, msgs, pk, sk, sig = batch
    assert api.EDDILITHIUM3_SIZES == dict(seed=57, pk=2009, sk=4057, sig=3407)
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
