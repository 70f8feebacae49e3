"""Worker of tests/test_gpu_rare_paths.py: ML-KEM and round-3 Kyber on the keys of tests/golden/rare_paths.json.gz whose matrix streams need a
fourth SHAKE128 block (at every position of the matrix, several in one key, and the 255 / 256 boundaries at the end of block 3) and on
encapsulation keys whose t^ is saturated (tests/rare_inputs.py), byte for byte against the oracle.  The test imports it for the default
routes and runs it in a process of its own under each environment of test_gpu_round3.py::test_kem_batch_routes, which forces the other
batch routes at these sizes.
    python tests/kem_rare_worker.py <param> [<param> ...]"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rare_inputs as ri  # noqa: E402
from conftest import hx, load_golden  # noqa: E402
from circl_amd import hostapi  # noqa: E402
from oracle import orc  # noqa: E402

PLACES = (0, 1, 63, 64, -1)   # where the special items of a mixed batch go: both ends of a wavefront's worth of items and of the batch


def _rows(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), -1).copy()


def arrangements(scheme, param):
    """-> [(name, seeds (n, 64), rho expected per item or None)]"""
    K = ri.KEM[param][0]
    f = load_golden("rare_paths.json.gz")["kem_fourth_block"][scheme][str(K)]
    every = f["positions"] + [f["multi"], f["exactly_255"]]
    out = [("every item has a fourth block", _rows([hx(r["seed"]) for r in every]), [r["rho"] for r in every])]
    # (the 64 seeds in between are chosen so that none of their streams needs one: tests/test_oracle_rare_paths.py counts them)
    out.append(("only the first and the last item",) + ri.kem_only_the_ends(scheme, param, f))
    side = f["positions"] + [f["exactly_256"]]
    out.append(("every position side by side", _rows([hx(r["seed"]) for r in side]), [r["rho"] for r in side]))
    return out


def fourth_block(param):
    checks = 0
    for name, seeds, rhos in arrangements("mlkem", param):
        n = len(seeds)
        rng = np.random.default_rng(n)
        ek0, dk0 = orc.mlkem_keygen(param, seeds)
        ek, dk = hostapi.mlkem_keygen(param, seeds)
        assert (ek == ek0).all() and (dk == dk0).all(), ("keygen", param, name)
        assert all(r is None or ek[i, -32:].tobytes().hex() == r for i, r in enumerate(rhos)), ("rho", param, name)
        m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ct0, ss0, _ = orc.mlkem_encaps(param, ek, m)
        ct, ss, st = hostapi.mlkem_encaps(param, ek, m)
        assert not st.any() and (ct == ct0).all() and (ss == ss0).all(), ("encaps", param, name)
        got, st = hostapi.mlkem_decaps(param, dk, ct)
        assert not st.any() and (got == ss0).all(), ("decaps", param, name)
        bad = ct.copy()
        bad[::2, 7] ^= 8                                                          # implicit rejection re-encrypts with the same matrix
        got, st = hostapi.mlkem_decaps(param, dk, bad)
        want, _ = orc.mlkem_decaps(param, dk, bad)
        assert not st.any() and (got == want).all(), ("decaps, rejected", param, name)
        for k in (0, n - 1):                                                      # one key for the batch
            ct1, ss1, st1 = hostapi.mlkem_encaps_shared(param, ek[k:k + 1], m)
            ct10, ss10, _ = orc.mlkem_encaps(param, np.tile(ek[k:k + 1], (n, 1)), m)
            assert not st1.any() and (ct1 == ct10).all() and (ss1 == ss10).all(), ("encaps, one key", param, name, k)
            got, st = hostapi.mlkem_decaps_shared(param, dk[k:k + 1], ct1)
            assert not st.any() and (got == ss10).all(), ("decaps, one key", param, name, k)
        idx = rng.permutation(n).astype(np.uint32)                               # a key table and an index vector
        pub, prv = hostapi.KeyTable("mlkem-public", param, ek), hostapi.KeyTable("mlkem-private", param, dk)
        ctt, sst, stt = pub.encaps(m, idx)
        ctt0, sst0, _ = orc.mlkem_encaps(param, ek[idx], m)
        assert not stt.any() and (ctt == ctt0).all() and (sst == sst0).all(), ("encaps, table", param, name)
        got, st = prv.decaps(ctt, idx)
        assert not st.any() and (got == sst0).all(), ("decaps, table", param, name)
        pub.close()
        prv.close()
        checks += 1
    for name, seeds, rhos in arrangements("kyber", param):                       # round-3 Kyber: per-item keys only
        n = len(seeds)
        rng = np.random.default_rng(100 + n)
        ek0, dk0 = orc.kyber_r3_keygen(param, seeds)
        ek, dk = hostapi.kyber_keygen(param, seeds)
        assert (ek == ek0).all() and (dk == dk0).all(), ("kyber keygen", param, name)
        assert all(r is None or ek[i, -32:].tobytes().hex() == r for i, r in enumerate(rhos)), ("kyber rho", param, name)
        es = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ct0, ss0 = orc.kyber_r3_encaps(param, ek, es)
        ct, ss = hostapi.kyber_encaps(param, ek, es)
        assert (ct == ct0).all() and (ss == ss0).all(), ("kyber encaps", param, name)
        bad = ct.copy()
        bad[::2, 7] ^= 8
        assert (hostapi.kyber_decaps(param, dk, bad) == orc.kyber_r3_decaps(param, dk, bad)).all(), ("kyber decaps", param, name)
        assert (hostapi.kyber_decaps(param, dk, ct) == ss0).all()
        checks += 1
    return checks


def _mixed_batches(param, scheme, families):
    """batches of 70 honest keys with five saturated ones each at PLACES -> [(ek (70, EK), [(place, family)])]"""
    K = ri.KEM[param][0]
    fix = load_golden("rare_paths.json.gz")["kem_fourth_block"][scheme][str(K)]
    rhos = [hashlib.sha3_256(b"saturated ek rho").digest(), hx(fix["multi"]["rho"])]       # a random one and one with fourth blocks
    todo = [(f, rho) for rho in rhos for f in families]
    n = 70
    out = []
    for b in range(0, len(todo), len(PLACES)):
        rng = np.random.default_rng(param + b)
        ek, _ = orc.mlkem_keygen(param, rng.integers(0, 256, (n, 64), dtype=np.uint8))
        placed = []
        for place, (fam, rho) in zip(PLACES, todo[b:b + len(PLACES)]):
            ek[place] = np.frombuffer(ri.saturated_ek(param, fam, rho), np.uint8)
            placed.append((place % n, fam))
        out.append((ek, placed))
    return out


def saturated_keys(param):
    checks = 0
    for ek, placed in _mixed_batches(param, "mlkem", ri.EK_FAMILIES + ri.EK_REFUSED):
        n = len(ek)
        rng = np.random.default_rng(n + len(placed))
        m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ct0, ss0, st0 = orc.mlkem_encaps(param, ek, m)
        refused = sorted(p for p, fam in placed if fam in ri.EK_REFUSED)
        assert np.flatnonzero(st0).tolist() == refused and (st0[refused] == 1).all()
        ct, ss, st = hostapi.mlkem_encaps(param, ek, m)
        assert (st == st0).all() and (ct == ct0).all() and (ss == ss0).all(), ("saturated, per item", param, placed)
        assert not ct[refused].any() and not ss[refused].any()
        idx = rng.permutation(n).astype(np.uint32)
        pub = hostapi.KeyTable("mlkem-public", param, ek)     # a public key's canonicity is reported per item (include/circl_hip.h)
        ctt, sst, stt = pub.encaps(m, idx)
        ctt0, sst0, stt0 = orc.mlkem_encaps(param, ek[idx], m)                    # (zero rows where it refuses)
        assert (stt == stt0).all() and (ctt == ctt0).all() and (sst == sst0).all(), ("saturated, table", param, placed)
        assert (stt0 == st0[idx]).all() and not ctt[stt == 1].any() and not sst[stt == 1].any()
        pub.close()
        for p, fam in placed:                                                     # one key for the batch: 65 messages
            ct1, ss1, st1 = hostapi.mlkem_encaps_shared(param, ek[p:p + 1], m[:65])
            ct10, ss10, st10 = orc.mlkem_encaps(param, np.tile(ek[p:p + 1], (65, 1)), m[:65])
            assert (st1 == st10).all() and (ct1 == ct10).all() and (ss1 == ss10).all(), ("saturated, one key", param, fam)
        checks += 1
    for ek, placed in _mixed_batches(param, "kyber", ri.EK_FAMILIES + ri.EK_NONCANONICAL):
        n = len(ek)
        es = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
        ct0, ss0 = orc.kyber_r3_encaps(param, ek, es)
        ct, ss = hostapi.kyber_encaps(param, ek, es)
        assert (ct == ct0).all() and (ss == ss0).all(), ("kyber saturated", param, placed)
        checks += 1
    return checks


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print("kem rare ok", p, fourth_block(int(p)), saturated_keys(int(p)))
