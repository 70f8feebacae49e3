"""Child process of the HPKE DHKEM chunk-boundary test (tests/test_gpu_hpke.py): CIRCL_HIP_HOST_CHUNK is read once per process, so the
run with small chunks needs a process of its own.

    python tests/hpke_worker.py KEM DEVICE IN.npz OUT.npz

IN holds ikmR, ikmS, ikmE (n, N); OUT gets the keys and, for the base and the auth mode, enc, ss, ok and the decapsulated ss2, ok2."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(kem, device, src, dst):
    from circl_amd import hostapi as api
    kem, device = int(kem, 0), int(device)
    d = np.load(src)
    skR, pkR = api.hpke_dhkem_derive_keypair(kem, d["ikmR"], device=device)
    skS, pkS = api.hpke_dhkem_derive_keypair(kem, d["ikmS"], device=device)
    enc, ss, ok = api.hpke_dhkem_encap(kem, pkR, d["ikmE"], device=device)
    ss2, ok2 = api.hpke_dhkem_decap(kem, skR, enc, device=device)
    aenc, ass, aok = api.hpke_dhkem_auth_encap(kem, pkR, skS, d["ikmE"], device=device)
    ass2, aok2 = api.hpke_dhkem_auth_decap(kem, skR, aenc, pkS, pkR=pkR, device=device)
    np.savez(dst, skR=skR, pkR=pkR, skS=skS, pkS=pkS, enc=enc, ss=ss, ok=ok, ss2=ss2, ok2=ok2, aenc=aenc, ass=ass, aok=aok, ass2=ass2, aok2=aok2)


if __name__ == "__main__":
    main(*sys.argv[1:5])
