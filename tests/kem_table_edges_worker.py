"""Worker of tests/test_gpu_keytable.py::test_mlkem_table_layout_at_its_padding_edges: key tables of G - 1, G and G + 1 entries
(G = entries per group of A^T rows: 16 / 7 / 4 for ML-KEM-512 / -768 / -1024 -- the rows are padded to whole groups, H(ek) and the
status bytes follow them) through the per-call key-table entry points and through resident tables, against the oracle.  A process of
its own, so that the environment chooses the resident tables' route (one launch / three launches).
    python tests/kem_table_edges_worker.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from circl_amd import hostapi  # noqa: E402
from oracle import orc  # noqa: E402

N = 40
for param, G in ((512, 16), (768, 7), (1024, 4)):
    for nkeys in (G - 1, G, G + 1):
        rng = np.random.default_rng(1000 * param + nkeys)
        ek, dk = orc.mlkem_keygen(param, rng.integers(0, 256, (nkeys, 64), dtype=np.uint8))
        ek[1, 0] = 0xff
        ek[1, 1] |= 0x0f                                  # public entry 1: first coefficient 0xfff >= q (cpapke.go:45-55)
        dk[nkeys - 2, -40] ^= 1                           # private entry nkeys - 2: stored H(ek) no longer matches (kem.ErrPrivKey)
        m = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        idx = rng.integers(0, nkeys, N).astype(np.uint32)
        idx[:4] = [nkeys - 1, 0, 1, nkeys - 2]
        zero = np.zeros(N, np.uint32)
        pub = hostapi.KeyTable("mlkem-public", param, ek)
        prv = hostapi.KeyTable("mlkem-private", param, dk)
        _, ks0 = orc.mlkem_decaps(param, dk, np.zeros((nkeys, hostapi.KEM_SIZES[param][2]), np.uint8))
        want_ks = [2 if i == nkeys - 2 else 0 for i in range(nkeys)]
        assert ks0.tolist() == want_ks and prv.key_status.tolist() == want_ks and not pub.key_status.any(), (param, nkeys, prv.key_status)
        for ix in (idx, zero):                            # zero: every item uses entry 0 (the resident tables: no index vector at all)
            ct0, ss0, st0 = orc.mlkem_encaps(param, ek[ix], m)
            assert (st0 == (ix == 1)).all()
            ctd = ct0.copy()
            ctd[::3, 11] ^= 8                             # implicit rejection for every third item
            ssd0, std0 = orc.mlkem_decaps(param, dk[ix], ctd)
            assert (std0 == 2 * (ix == nkeys - 2)).all()
            for form in ("keyed", "table"):
                if form == "keyed":
                    ct, ss, st = hostapi.mlkem_encaps_keyed(param, ek, ix, m)
                    ssd, std = hostapi.mlkem_decaps_keyed(param, dk, ix, ctd)
                else:
                    ct, ss, st = pub.encaps(m, ix if ix is idx else None)
                    ssd, std = prv.decaps(ctd, ix if ix is idx else None)
                where = (param, nkeys, form, ix is idx)
                assert (st == st0).all() and (ct == ct0).all() and (ss == ss0).all(), where
                assert (std == std0).all() and (ssd == ssd0).all(), where
        pub.close()
        prv.close()
print("kem table edges ok")
