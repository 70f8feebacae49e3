"""Child process of the Ed*-Dilithium* chunk-boundary tests (tests/test_gpu_eddilithium2.py, tests/test_gpu_eddilithium3.py): CIRCL_HIP_HOST_CHUNK is
read once per process, so the run with small chunks needs a process of its own.

    python tests/eddilithium_worker.py MODE IN.npz OUT.npz

IN holds seeds (n, seed bytes), blob and off (message i is blob[off[i]:off[i + 1]]); OUT gets pk, sk, sig and the verdicts ok."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(mode, src, dst):
    from circl_amd import hostapi
    keygen, sign, verify = (getattr(hostapi, "eddilithium%s_%s" % (mode, op)) for op in ("keygen", "sign", "verify"))
    d = np.load(src)
    msgs = [bytes(d["blob"][a:b]) for a, b in zip(d["off"][:-1], d["off"][1:])]
    pk, sk = keygen(d["seeds"])
    sig = sign(sk, msgs)
    np.savez(dst, pk=pk, sk=sk, sig=sig, ok=verify(pk, sig, msgs))


if __name__ == "__main__":
    main(*sys.argv[1:4])
