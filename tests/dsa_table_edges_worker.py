"""Worker of tests/test_gpu_keytable.py::test_mldsa_table_layout_at_its_padding_edges: public-key tables of IT - 1, IT and IT + 1 entries
(IT = items per workgroup, 64 / (K L): 4 / 2 / 1 for ML-DSA-44 / -65 / -87, 2 for Dilithium3 -- the packed A rows are padded to whole
groups of IT entries, a 64-byte tr slot per entry follows them; round 3 keeps its 32-byte tr in such a slot) through the per-call key
table and through resident tables, and tables of prepared private keys of the same sizes, against the oracle.  A process of its own, so
that the environment chooses the resident tables' route (one launch / the scratch route).
    python tests/dsa_table_edges_worker.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from circl_amd import hostapi  # noqa: E402
from oracle import orc  # noqa: E402

N = 24
for param, IT in ((44, 4), (65, 2), (87, 1), (3, 2)):
    r3 = param in (2, 3, 5)
    for nkeys in (IT - 1, IT, IT + 1):
        if nkeys == 0:
            continue
        rng = np.random.default_rng(1000 * param + nkeys)
        pk, sk = orc.mldsa_keygen(param, rng.integers(0, 256, (nkeys, 32), dtype=np.uint8))
        idx = rng.integers(0, nkeys, N).astype(np.uint32)
        idx[:2] = [nkeys - 1, 0]                          # the last entry is in use: an offset wrong by one padding group reads another key
        msgs = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 200, N)]
        msgs[0] = bytes(rng.integers(0, 256, 2500, dtype=np.uint8))   # > 2048 bytes: the long-message pre-pass reads the table's tr of entry nkeys - 1
        ctxs = None if r3 else [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 30, N)]
        pub = hostapi.KeyTable("mldsa-public", param, pk)
        prv = hostapi.KeyTable("mldsa-private", param, sk)
        for ix in (idx, np.zeros(N, np.uint32)):          # zeros: every item uses entry 0 (the resident table: no index vector at all)
            sig = hostapi.mldsa_sign(param, sk[ix], msgs, ctxs=ctxs)
            bad = sig.copy()
            bad[2::5, 9] ^= 4                             # every fifth signature is corrupted (items 0 and 1, the table's two ends, stay intact)
            want = orc.mldsa_verify(param, pk[ix], bad, msgs, ctxs=ctxs).astype(bool)
            assert want[:2].all() and want[3::5].all() and not want[2::5].any(), (param, nkeys)
            where = (param, nkeys, ix is idx)
            if ix is idx:
                assert (hostapi.mldsa_verify_keyed(param, pk, ix, bad, msgs, ctxs=ctxs).astype(bool) == want).all(), ("keyed",) + where
            ok = pub.verify(bad, msgs, ctxs=ctxs, key_idx=ix if ix is idx else None).astype(bool)
            assert (ok == want).all(), ("table",) + where
        # the prepared private keys: entry key_idx[i] signs item i, byte for byte the oracle's signature
        got = prv.sign(msgs, ctxs=ctxs, key_idx=idx)
        assert (got == orc.mldsa_sign(param, sk[idx], msgs, ctxs=ctxs)).all(), ("sign", param, nkeys)
        pub.close()
        prv.close()
print("dsa table edges ok")
