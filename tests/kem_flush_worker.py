"""Worker of tests/test_gpu_kem_flush.py: ML-KEM key generation, encapsulation and decapsulation on the inputs of tests/kem_flush_inputs.py
(matrix streams on the edges of the sampler's FIFO flush schedule, fourth-block stragglers), byte for byte against the oracle, at the batch
sizes 1, G - 1, G, G + 1 and 2 G + 3 -- per-item keys, one key for the batch, a key table.  The test imports it for the default routes and
runs it in a process of its own under each environment that forces another batch route at these sizes.
    python tests/kem_flush_worker.py <inputs.json> <param> [<param> ...]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import kem_flush_inputs as fi  # noqa: E402
from circl_amd import hostapi  # noqa: E402
from oracle import orc  # noqa: E402


def find_inputs():
    """-> {str(K): {"rho": {shape: hex}, "d": {shape: hex}}} (JSON-able: the test finds them once and hands them to every worker)"""
    return {str(K): {"rho": {s: v.hex() for s, v in fi.search(K, False).items()}, "d": {s: v.hex() for s, v in fi.search(K, True).items()}}
            for K in (2, 3, 4)}


def batches(param, inputs):
    """-> [(n, places, seeds (n, 64) whose placed items have a found d, ek (n, EK) whose placed items end in a found rho)]"""
    K = fi.PARAM_K[param]
    shapes = list(fi.SHAPES)
    rho = [bytes.fromhex(inputs[str(K)]["rho"][s]) for s in shapes]
    d = [bytes.fromhex(inputs[str(K)]["d"][s]) for s in shapes]
    out = []
    for b, (n, places) in enumerate(fi.placements(K, len(shapes))):
        rng = np.random.default_rng(1000 * param + b)
        ds = fi.ordinary(K, n, b)
        fill = np.frombuffer(b"".join(ds), np.uint8).reshape(n, 32)
        z = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ek, _ = orc.mlkem_keygen(param, np.concatenate([fill, z], axis=1))         # canonical t^, ordinary rho
        seeds = np.concatenate([fill, z], axis=1)
        for p, s in places.items():
            ek[p, -32:] = np.frombuffer(rho[s], np.uint8)
            seeds[p, :32] = np.frombuffer(d[s], np.uint8)
        out.append((n, places, seeds, ek))
    return out


def run(param, inputs):
    K = fi.PARAM_K[param]
    checks = 0
    for n, places, seeds, ek_over in batches(param, inputs):
        what = (param, n, sorted(places.items()))
        rng = np.random.default_rng(n + 7 * len(places))
        m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        # key generation from the found seeds, then decapsulation (its re-encryption samples the same matrix) with those keys
        ek0, dk0 = orc.mlkem_keygen(param, seeds)
        ek, dk = hostapi.mlkem_keygen(param, seeds)
        assert (ek == ek0).all() and (dk == dk0).all(), ("keygen",) + what
        for p, s in places.items():
            assert ek0[p, -32:].tobytes() == fi.mlkem_rho(K, seeds[p, :32].tobytes()), ("rho",) + what
        ct0, ss0, _ = orc.mlkem_encaps(param, ek0, m)
        ct, ss, st = hostapi.mlkem_encaps(param, ek0, m)
        assert not st.any() and (ct == ct0).all() and (ss == ss0).all(), ("encaps, generated keys",) + what
        bad = ct0.copy()
        bad[::2, 7] ^= 8                                                             # implicit rejection on every other item
        want, _ = orc.mlkem_decaps(param, dk0, bad)
        got, st = hostapi.mlkem_decaps(param, dk0, bad)
        assert not st.any() and (got == want).all() and (got[1::2] == ss0[1::2]).all(), ("decaps",) + what
        # encapsulation to oracle-made keys whose rho is overwritten with a found one
        cto, sso, sto = orc.mlkem_encaps(param, ek_over, m)
        ct, ss, st = hostapi.mlkem_encaps(param, ek_over, m)
        assert not sto.any() and not st.any() and (ct == cto).all() and (ss == sso).all(), ("encaps, rho overwritten",) + what
        # one key for the batch, and a key table with an index vector: every placed key
        for p in places:
            ct1, ss1, st1 = hostapi.mlkem_encaps_shared(param, ek_over[p:p + 1], m)
            ct10, ss10, _ = orc.mlkem_encaps(param, np.tile(ek_over[p:p + 1], (n, 1)), m)
            assert not st1.any() and (ct1 == ct10).all() and (ss1 == ss10).all(), ("encaps, one key", p) + what
            c1, s1, _ = orc.mlkem_encaps(param, np.tile(ek0[p:p + 1], (n, 1)), m)
            got, st = hostapi.mlkem_decaps_shared(param, dk0[p:p + 1], c1)
            assert not st.any() and (got == s1).all(), ("decaps, one key", p) + what
        idx = rng.permutation(n).astype(np.uint32)
        pub, prv = hostapi.KeyTable("mlkem-public", param, ek_over), hostapi.KeyTable("mlkem-private", param, dk0)
        ctt, sst, stt = pub.encaps(m, idx)
        ctt0, sst0, _ = orc.mlkem_encaps(param, ek_over[idx], m)
        assert not stt.any() and (ctt == ctt0).all() and (sst == sst0).all(), ("encaps, table",) + what
        c2, s2, _ = orc.mlkem_encaps(param, ek0[idx], m)
        got, st = prv.decaps(c2, idx)
        assert not st.any() and (got == s2).all(), ("decaps, table",) + what
        pub.close()
        prv.close()
        checks += 1
    return checks


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        found = json.load(f)
    for p in sys.argv[2:]:
        print("kem flush ok", p, run(int(p), found))
