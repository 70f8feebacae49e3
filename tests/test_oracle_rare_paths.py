"""CPU side of the rare-path and saturated-input tests: every property tests/golden/rare_paths.json.gz claims is recomputed here from
hashlib alone (or, for `sign_rejections`, from the oracle's signing trace), and the oracle itself is checked on the saturated inputs
against plain integer arithmetic (tests/rare_inputs.py) -- so that tests/test_gpu_rare_paths.py and tests/test_gpu_mldsa_extremes.py
can neither pass on a stale fixture nor lean on a reference that shares the kernels' reduction schedule.  No GPU."""
import hashlib

import numpy as np
import pytest

import rare_inputs as ri
from conftest import hx, load_golden
from oracle import orc

FIX = load_golden("rare_paths.json.gz")
KEM_K = {2: 512, 3: 768, 4: 1024}
DSA_PARAMS = (44, 65, 87, 2, 3, 5)


# ---- the samplers' streams, from hashlib -------------------------------------------------------------------------------------------------
def _rhoprime(param, xi):
    K, L = ri.DSA[param][:2]
    return hashlib.shake_256(xi + (bytes([K, L]) if param > 10 else b"")).digest(128)[32:96]   # dilithium.go:189-195; round 3 hashes xi alone


def _accepted_nibbles(param, xi, nonce, nbytes):
    """how many of the first 2 * nbytes nibbles of SHAKE256(rho' || LE16(nonce)) PolyDeriveUniformLeqEta accepts (sample.go:125-175)"""
    lim = 8 if ri.DSA[param][2] == 4 else 14
    buf = hashlib.shake_256(_rhoprime(param, xi) + nonce.to_bytes(2, "little")).digest(nbytes)
    return sum((b & 15) <= lim for b in buf) + sum((b >> 4) <= lim for b in buf)


def _accepted_in_3_blocks(rho, x, y):
    """how many of the 336 12-bit candidates in three SHAKE128 blocks of XOF(rho || x || y) are below q (sample.go:192-236)"""
    buf = hashlib.shake_128(rho + bytes([x, y])).digest(504)
    n = 0
    for k in range(0, 504, 3):
        n += ((buf[k] | buf[k + 1] << 8) & 0xFFF) < 3329
        n += (buf[k + 1] >> 4 | buf[k + 2] << 4) < 3329
    return n


def _kem_rho(scheme, K, d):
    return hashlib.sha3_512(d + (bytes([K]) if scheme == "mlkem" else b"")).digest()[:32]


# ---- fixture properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", [65, 3])
def test_eta4_seeds_need_a_third_block(param):
    hits = FIX["eta4_third_block"][str(param)]
    L = ri.DSA[param][1]
    assert len(hits) >= 4
    nonces = [n for h in hits for n in h["nonces"]]
    assert any(n < L for n in nonces) and any(n >= L for n in nonces)            # an s1 polynomial and an s2 polynomial
    for h in hits:
        xi = hx(h["xi"])
        assert xi == h["seed"].to_bytes(32, "little") and h["nonces"]
        for n, c in zip(h["nonces"], h["accepted_in_544"]):
            assert _accepted_nibbles(param, xi, n, 272) == c < 256


def test_eta4_seeds_of_the_issue_are_third_block_seeds():
    # the three hits measured when the gap was found: integer seeds 10063, 14708 and 28918 with nonces 9, 6 and 10 (ML-DSA-65)
    for seed, nonce in ((10063, 9), (14708, 6), (28918, 10)):
        assert _accepted_nibbles(65, seed.to_bytes(32, "little"), nonce, 272) < 256
    assert {10063, 14708, 28918} <= {h["seed"] for h in FIX["eta4_third_block"]["65"]}


@pytest.mark.parametrize("param", [44, 87])
def test_eta2_seeds_sit_on_the_block_1_boundary(param):
    f = FIX["eta2_second_block"][str(param)]
    K, L = ri.DSA[param][:2]
    for kind, ok in (("inside_block1", lambda c: c >= 257), ("exactly_256", lambda c: c == 256), ("exactly_255", lambda c: c == 255)):
        assert {h["nonce"] for h in f[kind]} == {0, L, K + L - 1}                # first of s1, first and last of s2
        for h in f[kind]:
            c = _accepted_nibbles(param, hx(h["xi"]), h["nonce"], 136)
            assert c == h["accepted_in_272"] and ok(c), (kind, h)


@pytest.mark.parametrize("scheme", ["mlkem", "kyber"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_kem_rhos_need_a_fourth_block_where_they_say(scheme, K):
    f = FIX["kem_fourth_block"][scheme][str(K)]
    recs = f["positions"] + [f["multi"], f["exactly_256"], f["exactly_255"]]
    for r in recs:
        seed, rho = hx(r["seed"]), hx(r["rho"])
        assert len(seed) == 64 and seed[:32] == r["d"].to_bytes(32, "little") and _kem_rho(scheme, K, seed[:32]) == rho
        cnt = {(x, y): _accepted_in_3_blocks(rho, x, y) for x in range(K) for y in range(K)}
        assert sorted(r["fourth"]) == sorted([x, y] for (x, y), c in cnt.items() if c < 256)
        if "accepted_in_336" in r:
            assert cnt[tuple(r["xy"])] == r["accepted_in_336"]
    assert [p["xy"] for p in f["positions"]] == [[x, y] for x in range(K) for y in range(K)]     # every stream of the matrix
    assert all(p["xy"] in p["fourth"] for p in f["positions"])
    assert len(f["multi"]["fourth"]) >= 2
    assert f["exactly_256"]["accepted_in_336"] == 256 and f["exactly_255"]["accepted_in_336"] == 255
    assert f["exactly_255"]["xy"] in f["exactly_255"]["fourth"] and f["exactly_256"]["xy"] not in f["exactly_256"]["fourth"]
    # the oracle's keygen puts that rho into the key
    kg = orc.mlkem_keygen if scheme == "mlkem" else orc.kyber_r3_keygen
    ek, _ = kg(KEM_K[K], np.frombuffer(b"".join(hx(r["seed"]) for r in recs), np.uint8).reshape(-1, 64))
    assert [e[-32:].tobytes().hex() for e in ek] == [r["rho"] for r in recs]


@pytest.mark.parametrize("scheme", ["mlkem", "kyber"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_kem_batch_with_fourth_blocks_only_at_its_ends(scheme, K):
    # the batch the GPU tests call "only the first and the last item": exactly items 0 and n - 1 have a stream that needs a fourth block
    seeds, rhos = ri.kem_only_the_ends(scheme, KEM_K[K], FIX["kem_fourth_block"][scheme][str(K)])
    n = len(seeds)
    needs = []
    for i in range(n):
        rho = _kem_rho(scheme, K, seeds[i, :32].tobytes())
        assert rhos[i] is None or rho.hex() == rhos[i]
        if any(_accepted_in_3_blocks(rho, x, y) < 256 for x in range(K) for y in range(K)):
            needs.append(i)
    assert n == 66 and needs == [0, n - 1]
    assert len({bytes(r) for r in seeds}) == n


@pytest.mark.parametrize("param", [65, 3])
def test_eta4_mixed_batches_have_third_blocks_only_where_placed(param):
    # the batches of tests/test_gpu_rare_paths.py::test_mldsa_keygen_on_rare_sampler_seeds: only the placed seeds need a third block
    K, L = ri.DSA[param][:2]
    for seeds, put in ri.dsa_mixed_batches(FIX, param):
        needs = [i for i in range(len(seeds)) if any(_accepted_nibbles(param, seeds[i].tobytes(), nonce, 272) < 256 for nonce in range(K + L))]
        assert needs == sorted(p for p, _ in put), len(seeds)


def _sign_key(param):
    f = FIX["sign_rejections"][str(param)]
    _, sk = orc.mldsa_keygen(param, np.frombuffer(hx(f["xi"]), np.uint8))
    return f, sk[0].tobytes()


@pytest.mark.parametrize("param", DSA_PARAMS)
def test_sign_rejection_items_take_the_chains_they_record(param):
    f, sk = _sign_key(param)
    items = f["items"]
    seen = {c: 0 for c in orc.SIGN_CAUSES}
    for it in items:
        sig, att, causes = orc.mldsa_sign_trace(param, sk, hx(it["msg"]))
        assert (att, causes) == (it["attempts"], it["causes"]) and len(causes) == att - 1 and len(hx(it["msg"])) <= 64
        assert sig == orc.mldsa_sign_one(param, sk, hx(it["msg"]))
        for c in causes:
            seen[c] += 1
    att = [it["attempts"] for it in items]
    assert sum(a >= 20 for a in att) >= 3 and 1 in att and max(att) < 200
    assert min(seen[1], seen[2], seen[4]) >= 3, seen


@pytest.mark.parametrize("param", DSA_PARAMS)
def test_ct0_rejections_need_a_saturated_t0(param):
    """The |c t0| check cannot reject with a key KeyGen made at tau 2^12 < gamma2 (ML-DSA-65 / -87, Dilithium3 / 5), and does so about
    once in 1e7 attempts at ML-DSA-44 / Dilithium2 (a 6.4 sigma sum); the fixture reaches it through sk's own t0 field, every
    coefficient 2^12 (bytes 0x00) or -2^12 + 1 (0xFF), where tau = 39 -- and records that the other sets never take it even then."""
    tau, gamma2 = {44: (39, 95232), 65: (49, 261888), 87: (60, 261888), 2: (39, 95232), 3: (49, 261888), 5: (60, 261888)}[param]
    f, sk = _sign_key(param)
    assert not any(3 in it["causes"] for it in f["items"])
    n3 = {0x00: 0, 0xFF: 0}
    for it in f["t0_saturated"]:
        key = ri.sk_with_t0_bytes(param, sk, it["t0_byte"])
        sig, att, causes = orc.mldsa_sign_trace(param, key, hx(it["msg"]))
        assert (att, causes) == (it["attempts"], it["causes"]) and att < 200
        assert sig == orc.mldsa_sign_one(param, key, hx(it["msg"]))
        n3[it["t0_byte"]] += causes.count(3)
    for byte in n3:
        att = [it["attempts"] for it in f["t0_saturated"] if it["t0_byte"] == byte]
        assert 1 in att and max(att) >= 20
    if tau * 4096 >= gamma2:
        assert min(n3.values()) >= 3, n3
    else:
        assert not any(n3.values())


# ---- the signing trace is the signer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,param", [("ML-DSA-44", 44), ("ML-DSA-65", 65), ("ML-DSA-87", 87)])
def test_sign_trace_gives_the_acvp_signatures(name, param):
    cases = load_golden("mldsa_acvp.json.gz")[name]["siggen"]
    assert len(cases) == 20
    for c in cases:
        sig, att, causes = orc.mldsa_sign_trace(param, hx(c["sk"]), hx(c["message"]), rnd=hx(c["rnd"]), internal=True)
        assert hashlib.sha256(sig).hexdigest() == c["sig_sha256"]
        assert sig == orc.mldsa_sign_one(param, hx(c["sk"]), hx(c["message"]), rnd=hx(c["rnd"]), internal=True)
        assert att >= 1 and len(causes) == att - 1 and set(causes) <= set(orc.SIGN_CAUSES)


# ---- saturated encapsulation keys: two oracles and plain integers -------------------------------------------------------------------------
def _ek_rhos(scheme, K):
    return [hashlib.sha3_256(b"saturated ek rho").digest(), hx(FIX["kem_fourth_block"][scheme][str(K)]["multi"]["rho"])]


def test_exact_transforms_are_the_oracle_transforms():
    rng = np.random.default_rng(2)
    p = rng.integers(0, ri.KQ, 256)
    assert (ri.kyber_ntt_exact(p) == orc.kyber_normalize(orc.kyber_ntt(p.astype(np.int16)))).all()
    assert (ri.kyber_ntt_exact(ri.kyber_ntt_exact(p), inverse=True) == p).all()
    p = rng.integers(0, ri.DQ, 256)
    assert (ri.dilithium_ntt_exact(p) == orc.dilithium_normalize(orc.dilithium_ntt(p.astype(np.uint32)))).all()
    assert (ri.dilithium_ntt_exact(ri.dilithium_ntt_exact(p), inverse=True) == p).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_mlkem_oracles_agree_on_saturated_keys(K):
    param = KEM_K[K]
    rng = np.random.default_rng(K)
    for rho in _ek_rhos("mlkem", K):
        fams = ri.EK_FAMILIES + ri.EK_REFUSED
        ek = np.frombuffer(b"".join(ri.saturated_ek(param, f, rho) for f in fams), np.uint8).reshape(len(fams), -1)
        m = rng.integers(0, 256, (len(fams), 32), dtype=np.uint8)
        ct, ss, st = orc.mlkem_encaps(param, ek, m)
        assert st.tolist() == [0] * len(ri.EK_FAMILIES) + [1] * len(ri.EK_REFUSED)
        assert not ct[st == 1].any() and not ss[st == 1].any()
        for i, f in enumerate(ri.EK_FAMILIES):                                    # big-integer K-PKE.Encrypt: one item per family
            ct_d, ss_d = ri.mlkem_encaps_direct(param, ek[i].tobytes(), m[i].tobytes())
            assert ct_d == ct[i].tobytes() and ss_d == ss[i].tobytes(), f


@pytest.mark.parametrize("K", [3, 4])
def test_vector_oracle_agrees_on_saturated_keys(K):
    # oracle/vec serves ML-KEM-768 and -1024 only, and needs AVX2; ML-KEM-512 has the scalar oracle and the plain integers above
    if not orc.vec_isa():
        pytest.skip("the vector oracle needs AVX2: its agreement with the scalar oracle on saturated keys is NOT checked on this machine")
    param = KEM_K[K]
    rng = np.random.default_rng(K)
    for rho in _ek_rhos("mlkem", K):
        fams = ri.EK_FAMILIES + ri.EK_REFUSED
        ek = np.frombuffer(b"".join(ri.saturated_ek(param, f, rho) for f in fams), np.uint8).reshape(len(fams), -1)
        m = rng.integers(0, 256, (len(fams), 32), dtype=np.uint8)
        ct, ss, st = orc.mlkem_encaps(param, ek, m)
        ctv, ssv, stv = orc.mlkem_encaps_vec(param, ek, m)
        assert (stv == st).all() and (ctv == ct).all() and (ssv == ss).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_kyber_r3_oracle_reduces_saturated_and_noncanonical_keys(K):
    param = KEM_K[K]
    rng = np.random.default_rng(10 + K)
    for rho in _ek_rhos("kyber", K):
        fams = ri.EK_FAMILIES + ri.EK_NONCANONICAL
        ek = np.frombuffer(b"".join(ri.saturated_ek(param, f, rho) for f in fams), np.uint8).reshape(len(fams), -1)
        seeds = rng.integers(0, 256, (len(fams), 32), dtype=np.uint8)
        ct, ss = orc.kyber_r3_encaps(param, ek, seeds)
        for i, f in enumerate(fams):
            ct_d, ss_d = ri.kyber_r3_encaps_direct(param, ek[i].tobytes(), seeds[i].tobytes())
            assert ct_d == ct[i].tobytes() and ss_d == ss[i].tobytes(), f


# ---- saturated ML-DSA keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", DSA_PARAMS)
def test_oracle_signs_and_verifies_with_saturated_keys(param):
    for fill in ri.S_FILLS:
        s1, s2 = ri.saturated_s(param, fill)
        pk, sk = ri.mldsa_key_from_s(param, s1, s2)
        msgs, att = ri.signable(param, sk, 4)
        assert max(att) < 200
        sig = orc.mldsa_sign(param, np.tile(np.frombuffer(sk, np.uint8), (4, 1)), msgs)
        assert orc.mldsa_verify(param, np.tile(np.frombuffer(pk, np.uint8), (4, 1)), sig, msgs).all(), fill     # the key is consistent
        for t0 in (4096, -4095):                                                # an inconsistent sk: sign only
            _, bad = ri.mldsa_key_from_s(param, s1, s2, t0_override=t0)
            assert bad == ri.sk_with_t0_bytes(param, sk, 0x00 if t0 == 4096 else 0xFF)
            assert max(ri.signable(param, bad, 2)[1]) < 200


@pytest.mark.parametrize("param", DSA_PARAMS)
def test_oracle_decodes_noncanonical_eta_codes_as_the_reference_does(param):
    # pack.go:9-37 PolyUnpackLeqEta: coefficient = q + eta - code, whatever the code; nothing is refused.  A code above 2 eta is the
    # coefficient eta - code < -eta: the key built in integers from THOSE s1, s2 has the non-canonical codes in its sk and a public key
    # that fits them, so the oracle's signature verifies exactly when the oracle decoded the codes that way.
    eta = ri.DSA[param][2]
    top = 7 if eta == 2 else 15
    s1, s2 = ri.saturated_s(param, "plus_eta")
    pk, sk = ri.mldsa_key_from_s(param, s1 - top, s2 - top)                       # every coefficient eta - top
    assert sk == ri.sk_with_eta_codes(param, sk, top, 1)
    msgs, att = ri.signable(param, sk, 3)
    assert max(att) < 200
    sig = orc.mldsa_sign(param, np.tile(np.frombuffer(sk, np.uint8), (3, 1)), msgs)
    assert orc.mldsa_verify(param, np.tile(np.frombuffer(pk, np.uint8), (3, 1)), sig, msgs).all()
