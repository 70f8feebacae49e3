"""Worker of tests/test_gpu_hybrid448.py: one fresh process per X448 KeyGen route (CIRCL_HIP_X448_KEYGEN in the environment).

    python tests/x448_route_worker.py OUT.npz

Runs circl_hip_x448_dev KeyGen on N_KEYGEN fixed scalars and a Kyber768-X448 encapsulation (the pair kernel) on N_ENCAPS fixed
keys / seeds, and saves the outputs; the parent compares the routes' files byte for byte."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_KEYGEN, N_ENCAPS = 193, 65


def inputs():
    rng = np.random.default_rng(448)
    return (rng.integers(0, 256, (N_KEYGEN, 56), dtype=np.uint8), rng.integers(0, 256, (N_ENCAPS, 64), dtype=np.uint8),
            rng.integers(0, 256, (N_ENCAPS, 56), dtype=np.uint8))


def main():
    import torch
    from circl_amd import device, hostapi
    k, seeds, eseeds = inputs()
    pub, ok = device.x448(torch.from_numpy(k).cuda())
    torch.cuda.synchronize()
    pk, _ = hostapi.hybrid_keygen(hostapi.KYBER768_X448, seeds)
    ct, ss, st = hostapi.hybrid_encaps(hostapi.KYBER768_X448, pk, eseeds)
    np.savez(sys.argv[1], route=os.environ.get("CIRCL_HIP_X448_KEYGEN", ""), pub=pub.cpu().numpy(), ok=ok.cpu().numpy(), pk=pk, ct=ct, ss=ss, st=st)


if __name__ == "__main__":
    main()
