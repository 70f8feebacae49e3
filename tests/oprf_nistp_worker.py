"""Child process of the P-256 / P-384 host-pipeline test (tests/test_gpu_oprf_nistp.py): the pipeline's chunk size (CIRCL_HIP_HOST_CHUNK) is
read once per process, so a run with small chunks needs a process of its own.

    python tests/oprf_nistp_worker.py CURVE DEVICE N OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODE = 1
DST = b"oprf_nistp_worker"
ORDER = {256: 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551,
         384: 0xffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973}


def inputs(curve, n):
    """(seeds, infos, inputs, blinds) of n items: inputs of i % 41 bytes (empty ones at both sides of the chunk boundary 255 | 256), infos
    of i % 7 bytes, blinds below the group order"""
    ns = curve // 8
    rng = np.random.default_rng(9497 + curve)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    infos = [rng.bytes(i % 7) for i in range(n)]
    ins = [rng.bytes(0 if i in (255, 256) else i % 41) for i in range(n)]
    blinds = np.frombuffer(b"".join((1 + int.from_bytes(rng.bytes(ns), "big") % (ORDER[curve] - 1)).to_bytes(ns, "big") for _ in range(n)), np.uint8)
    return seeds, infos, ins, blinds.reshape(n, ns).copy()


def run(api, curve, device, n):
    """every host form once: keys per item, one of them (item 0's) as the server's shared key"""
    seeds, infos, ins, blinds = inputs(curve, n)
    g = api.NistpOprf(curve, device=device)
    o = {}
    o["sk"], o["pk"], o["ok_keys"] = g.derive_keypair(MODE, seeds, infos)
    key = o["sk"][0].tobytes()
    o["blinded"], o["ok_blind"] = g.blind(MODE, ins, blinds)
    o["evaluated"], o["ok_eval"] = g.evaluate(key, o["blinded"])
    o["evaluated_own"], o["ok_eval_own"] = g.evaluate(o["sk"], o["blinded"])
    o["output"], o["ok_fin"] = g.finalize(ins, blinds, o["evaluated"])
    o["full"], o["ok_full"] = g.full_evaluate(MODE, key, ins)
    o["h2g"] = g.hash_to_group(ins, DST)
    o["h2g_nu"] = g.hash_to_group(ins, DST, nonuniform=True)
    o["h2s"] = g.hash_to_scalar(ins, DST)
    o["unblinded"], o["ok_mult"] = g.scalar_mult(blinds, o["blinded"], invert=True)
    o["pk_again"], o["ok_base"] = g.scalar_mult(o["sk"])
    return o


def main(curve, device, n, dst):
    from circl_amd import hostapi as api
    np.savez(dst, **run(api, int(curve), int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:5])
