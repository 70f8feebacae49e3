"""Child process of the OPRF host-pipeline tests (tests/test_gpu_oprf.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_ZEROCOPY_KB, CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/oprf_worker.py DEVICE N OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODE = 1
DST = b"oprf_worker-ristretto255"
ORDER = 2**252 + 27742317777372353535851937790883648493


def inputs(n):
    """(seeds, infos, inputs, blinds) of n items: inputs of i % 41 bytes (empty ones at both sides of the chunk boundary 255 | 256), infos
    of i % 7 bytes, blinds below the group order"""
    rng = np.random.default_rng(9497)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    infos = [rng.bytes(i % 7) for i in range(n)]
    ins = [rng.bytes(0 if i in (255, 256) else i % 41) for i in range(n)]
    blinds = np.frombuffer(b"".join((1 + int.from_bytes(rng.bytes(32), "little") % (ORDER - 1)).to_bytes(32, "little") for _ in range(n)), np.uint8)
    return seeds, infos, ins, blinds.reshape(n, 32).copy()


def run(api, device, n):
    """every host form once: keys per item, one of them (item 0's) as the server's shared key"""
    seeds, infos, ins, blinds = inputs(n)
    o = {}
    o["sk"], o["pk"], o["ok_keys"] = api.oprf_derive_keypair(MODE, seeds, infos, device=device)
    key = o["sk"][0].tobytes()
    o["blinded"], o["ok_blind"] = api.oprf_blind(MODE, ins, blinds, device=device)
    o["evaluated"], o["ok_eval"] = api.oprf_evaluate(key, o["blinded"], device=device)
    o["evaluated_own"], o["ok_eval_own"] = api.oprf_evaluate(o["sk"], o["blinded"], device=device)
    o["output"], o["ok_fin"] = api.oprf_finalize(ins, blinds, o["evaluated"], device=device)
    o["full"], o["ok_full"] = api.oprf_full_evaluate(MODE, key, ins, device=device)
    o["h2g"] = api.ristretto255_hash_to_group(ins, DST, device=device)
    o["h2s"] = api.ristretto255_hash_to_scalar(ins, DST, device=device)
    o["unblinded"], o["ok_mult"] = api.ristretto255_scalar_mult(blinds, o["blinded"], invert=True, device=device)
    o["pk_again"], o["ok_base"] = api.ristretto255_scalar_mult(o["sk"], device=device)
    return o


def main(device, n, dst):
    from circl_amd import hostapi as api
    np.savez(dst, **run(api, int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
