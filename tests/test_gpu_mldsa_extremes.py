"""Batch ML-DSA / Dilithium signing where the rejection loop and the ring arithmetic are pushed: the messages of
tests/golden/rare_paths.json.gz (every rejection cause, chains of 20 and more attempts -- the attempt counts are the oracle's, pinned in
tests/test_oracle_rare_paths.py, never the GPU's), private keys whose s1, s2 sit at +-eta in every coefficient and whose t0 sits at the
ends of its range, and non-canonical eta codes, which the reference decodes as q + eta - code and never refuses (pack.go:9-37).
Every signature is the oracle's, byte for byte."""
import numpy as np
import pytest

import rare_inputs as ri
from conftest import hx, load_golden
from circl_amd import hostapi
from oracle import orc

pytestmark = pytest.mark.gpu

FIX = load_golden("rare_paths.json.gz")
PARAMS = (44, 65, 87, 2, 3, 5)


def _rows(key, n):
    return np.tile(np.frombuffer(key, np.uint8), (n, 1))


def _key(param):
    f = FIX["sign_rejections"][str(param)]
    pk, sk = orc.mldsa_keygen(param, np.frombuffer(hx(f["xi"]), np.uint8))
    return f, pk[0].tobytes(), sk[0].tobytes()


@pytest.mark.parametrize("param", PARAMS)
def test_sign_rejection_chains_match_the_oracle(param):
    f, pk, sk = _key(param)
    msgs = [hx(it["msg"]) for it in f["items"]]
    n = len(msgs)
    want = orc.mldsa_sign(param, _rows(sk, n), msgs)
    assert orc.mldsa_verify(param, _rows(pk, n), want, msgs).all()
    assert (hostapi.mldsa_sign(param, _rows(sk, n), msgs) == want).all()                    # per-item keys, the same one n times
    got = hostapi.mldsa_sign_shared(param, sk, msgs)
    assert (got == want).all()
    assert hostapi.mldsa_verify(param, _rows(pk, n), got, msgs).all() and hostapi.mldsa_verify_shared(param, pk, got, msgs).all()
    _, others = orc.mldsa_keygen(param, np.random.default_rng(param).integers(0, 256, (2, 32), dtype=np.uint8))
    table = hostapi.KeyTable("mldsa-private", param, np.concatenate([others[:1], _rows(sk, 1), others[1:]]))
    assert (table.sign(msgs, key_idx=np.ones(n, np.uint32)) == want).all()                   # a table of prepared keys and an index vector
    table.close()
    one = hostapi.KeyTable("mldsa-private", param, sk)
    assert (one.sign(msgs) == want).all()
    one.close()
    # the |c t0| rejections: the same key with a saturated t0 (no public key fits it: signatures only)
    for byte in (0x00, 0xFF):
        bad = ri.sk_with_t0_bytes(param, sk, byte)
        m = [hx(it["msg"]) for it in f["t0_saturated"] if it["t0_byte"] == byte]
        want = orc.mldsa_sign(param, _rows(bad, len(m)), m)
        assert (hostapi.mldsa_sign(param, _rows(bad, len(m)), m) == want).all(), byte
        assert (hostapi.mldsa_sign_shared(param, bad, m) == want).all(), byte


@pytest.mark.parametrize("param,shared", [(44, False), (65, False), (87, True), (2, True), (3, True), (5, True)])
def test_sign_rejection_chains_inside_speculative_rounds(param, shared):
    # 3000 items take the batched rounds with k = 1, 2, 3, ... speculative attempts per item (test_sign_speculative_rounds_match_oracle);
    # the long chains sit at both ends and in the middle and outlast every other item, the remaining fixture items follow the first one
    f, pk, sk = _key(param)
    n = 3000
    rng = np.random.default_rng(3000 + param)
    msgs = [rng.integers(0, 256, 1 + (i % 60), dtype=np.uint8).tobytes() for i in range(n)]
    long_ = [hx(it["msg"]) for it in f["items"] if it["attempts"] >= 20][:3]
    rest = [hx(it["msg"]) for it in f["items"] if hx(it["msg"]) not in long_]
    for place, m in zip((0, 1499, 2999), long_):
        msgs[place] = m
    msgs[1:1 + len(rest)] = rest
    want = orc.mldsa_sign(param, _rows(sk, n), msgs)
    got = hostapi.mldsa_sign_shared(param, sk, msgs) if shared else hostapi.mldsa_sign(param, _rows(sk, n), msgs)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad[:10].tolist()


@pytest.mark.parametrize("param", PARAMS)
def test_saturated_private_keys(param):
    # s1, s2 with every coefficient +eta, -eta, alternating: valid keys (t = A s1 + s2 in integers, tests/rare_inputs.py) no KeyGen ever returns
    keys = [ri.mldsa_key_from_s(param, *ri.saturated_s(param, fill)) for fill in ri.S_FILLS]
    pks, sks, msgs = [], [], []
    for pk, sk in keys:
        m, att = ri.signable(param, sk, 16)
        assert max(att) < 200
        want = orc.mldsa_sign(param, _rows(sk, 16), m)
        got = hostapi.mldsa_sign_shared(param, sk, m)
        assert (got == want).all()
        assert hostapi.mldsa_verify_shared(param, pk, got, m).all()
        assert (hostapi.mldsa_public_from_private(param, sk) == np.frombuffer(pk, np.uint8)).all()
        pks += [pk] * 16; sks += [sk] * 16; msgs += m
    pks, sks = np.frombuffer(b"".join(pks), np.uint8).reshape(48, -1), np.frombuffer(b"".join(sks), np.uint8).reshape(48, -1)
    got = hostapi.mldsa_sign(param, sks, msgs)                                             # the three keys in one batch, per-item keys
    assert (got == orc.mldsa_sign(param, sks, msgs)).all()
    assert hostapi.mldsa_verify(param, pks, got, msgs).all()
    assert orc.mldsa_verify(param, pks, got, msgs).all()                                  # the oracle accepts the GPU's signatures


@pytest.mark.parametrize("param", PARAMS)
def test_saturated_t0_in_the_private_key(param):
    # every t0 coefficient 2^12, then -2^12 + 1, under saturated s1, s2: no public key matches, the signature must still be the oracle's
    sks, msgs = [], []
    for fill in ri.S_FILLS:
        for t0 in (4096, -4095):
            _, sk = ri.mldsa_key_from_s(param, *ri.saturated_s(param, fill), t0_override=t0)
            m, att = ri.signable(param, sk, 6)
            assert max(att) < 200
            assert (hostapi.mldsa_sign_shared(param, sk, m) == orc.mldsa_sign(param, _rows(sk, 6), m)).all(), (fill, t0)
            sks += [sk] * 6; msgs += m
    sks = np.frombuffer(b"".join(sks), np.uint8).reshape(len(msgs), -1)
    assert (hostapi.mldsa_sign(param, sks, msgs) == orc.mldsa_sign(param, sks, msgs)).all()


@pytest.mark.parametrize("param", PARAMS)
def test_noncanonical_eta_codes_in_the_private_key(param):
    # codes 5..7 (eta = 2) / 9..15 (eta = 4) decode to coefficients below -eta (q + eta - code mod q); the reference signs with them.
    # Each code in a handful of coefficients (every 401st of the (K + L) * 256) and in all of them.
    f, pk, sk = _key(param)
    eta = ri.DSA[param][2]
    sks, msgs = [], []
    for code in range(2 * eta + 1, 8 if eta == 2 else 16):
        for every in (401, 1):
            key = ri.sk_with_eta_codes(param, sk, code, every)
            assert key != sk
            m, att = ri.signable(param, key, 3)
            assert max(att) < 200
            sks += [key] * 3; msgs += m
    sks = np.frombuffer(b"".join(sks), np.uint8).reshape(len(msgs), -1)
    want = orc.mldsa_sign(param, sks, msgs)
    got = hostapi.mldsa_sign(param, sks, msgs)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad.tolist()
    for k in (len(msgs) - 6, len(msgs) - 3):                                              # the top code: a handful, all of them; one key for its batch
        assert (hostapi.mldsa_sign_shared(param, sks[k], msgs[k:k + 3]) == want[k:k + 3]).all()
