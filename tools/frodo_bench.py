#!/usr/bin/env python3
"""Batch FrodoKEM-640-SHAKE rates on one GPU: prints ONE JSON record.

    python tools/frodo_bench.py [--sizes 8,10,12,14,16] [--host-size 12] [--repeats 5] [--window-ms 300] [--waves 10,5,2]

device_resident: the _dev entry points on torch buffers (inputs resident in HBM), timed with device events around enough
back-to-back calls to fill `window-ms` after a warm-up, `repeats` times; the record holds the median rate and the spread
(min, max).  waves: the same at the largest size for each matrix-workgroup split (CIRCL_HIP_FRODO_WAVES), alternated.
keccak: two yardsticks taken in the same process --
  host_call   circl_hip_keccak_f1600 on host buffers: 400 bytes cross the bus per permutation, so it measures the bus;
  on_chip     circl_hip_profile_valu_probe's Keccak-round instruction rate x SIMDs x 64 lanes / 4320 instructions per permutation:
              what the per-lane Keccak sustains with the states in registers.
fraction_of_keccak: each operation's rate over (yardstick / permutations per operation: 5301 keygen, 5360 encaps, 5302 decaps).
host: the host-buffer entry points on numpy arrays at one size (wall clock).  parity: a sample of every batch against tests/frodo.py."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frodo as ref  # noqa: E402
from circl_amd import _native as nat  # noqa: E402
from circl_amd import device as dv  # noqa: E402
from circl_amd import hostapi  # noqa: E402

PERMS = {"keygen": 5301, "encaps": 5360, "decaps": 5302}


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _rates(fn, n, repeats, window_ms):
    fn()
    torch.cuda.synchronize()
    one = _window(fn, 1)                                  # second call: warm, sizes the window
    reps = max(1, int(window_ms / max(one, 1e-3)))
    r = sorted(n / (_window(fn, reps) / 1e3) for _ in range(repeats))
    return {"per_s": statistics.median(r), "min_per_s": r[0], "max_per_s": r[-1], "ms_per_batch": n / statistics.median(r) * 1e3, "calls_per_window": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,10,12,14,16")
    ap.add_argument("--host-size", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--waves", default="10,5,2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frodo_bench: no GPU")
    rng = np.random.default_rng(3)
    rec = {"tool": "tools/frodo_bench.py", "device": torch.cuda.get_device_name(0), "perms_per_op": PERMS, "device_resident": {}, "waves": {}}
    parity = True
    sizes = [int(x) for x in a.sizes.split(",") if x]

    def ops_for(n):
        d = dv.FrodoDevice(n)
        seeds = torch.from_numpy(rng.integers(0, 256, (n, 48), dtype=np.uint8)).cuda()
        mus = torch.from_numpy(rng.integers(0, 256, (n, 16), dtype=np.uint8)).cuda()
        d.keygen(seeds), d.encaps(d.pk, mus)
        torch.cuda.synchronize()
        return d, seeds, mus, {"keygen": lambda: d.keygen(seeds), "encaps": lambda: d.encaps(d.pk, mus), "decaps": lambda: d.decaps(d.sk, d.ct)}

    for lg in sizes:
        n = 1 << lg
        d, seeds, mus, ops = ops_for(n)
        row = {name: _rates(fn, n, a.repeats, a.window_ms) for name, fn in ops.items()}
        ss2 = d.decaps(d.sk, d.ct)
        parity &= bool((ss2 == d.ss).all())
        sh, mh, pkh, skh, cth, ssh = (t.cpu().numpy() for t in (seeds, mus, d.pk, d.sk, d.ct, d.ss))
        for i in rng.choice(n, 2, replace=False):
            pk, sk = ref.keygen(sh[i].tobytes())
            ct, ss = ref.encaps(pk, mh[i].tobytes())
            parity &= (pkh[i].tobytes(), skh[i].tobytes(), cth[i].tobytes(), ssh[i].tobytes()) == (pk, sk, ct, ss)
        rec["device_resident"]["2^%d" % lg] = row
        if lg == max(sizes):
            for rnd in range(2):                          # alternated: the splits see the same machine state
                for w in [int(x) for x in a.waves.split(",") if x]:
                    os.environ["CIRCL_HIP_FRODO_WAVES"] = str(w)
                    got = {name: _rates(fn, n, 3, a.window_ms) for name, fn in ops.items()}
                    rec["waves"].setdefault("waves=%d" % w, []).append({k: v["per_s"] for k, v in got.items()})
            os.environ.pop("CIRCL_HIP_FRODO_WAVES", None)
        del d, seeds, mus, ops
        torch.cuda.empty_cache()

    # the Keccak yardsticks, same process
    props = torch.cuda.get_device_properties(0)
    k_inst = dv.valu_probe(0, 4)[0]
    simds = props.multi_processor_count * 4
    on_chip = k_inst * simds * 64 / 4320.0
    st = rng.integers(0, 1 << 63, (1 << 20, 25), dtype=np.uint64)
    hostapi.keccak_f1600(st[:4096].copy())
    t0 = time.perf_counter()
    hostapi.keccak_f1600(st)
    host_call = len(st) / (time.perf_counter() - t0)
    rec["keccak"] = {"host_call_perms_per_s": host_call, "on_chip_perms_per_s": on_chip, "keccak_round_insts_per_s_per_simd": k_inst, "simds": simds}
    big = rec["device_resident"]["2^%d" % max(sizes)]
    rec["fraction_of_keccak"] = {name: {"on_chip": big[name]["per_s"] * PERMS[name] / on_chip, "host_call": big[name]["per_s"] * PERMS[name] / host_call}
                                 for name in PERMS}

    n = 1 << a.host_size
    seeds, mus = rng.integers(0, 256, (n, 48), dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8)
    hostapi.frodo640shake_keygen(seeds[:64])
    t = time.perf_counter(); pk, sk = hostapi.frodo640shake_keygen(seeds); t1 = time.perf_counter()
    ct, ss = hostapi.frodo640shake_encaps(pk, mus); t2 = time.perf_counter()
    ss2 = hostapi.frodo640shake_decaps(sk, ct); t3 = time.perf_counter()
    parity &= bool((ss == ss2).all())
    rec["host"] = {"2^%d" % a.host_size: {"keygen_per_s": n / (t1 - t), "encaps_per_s": n / (t2 - t1), "decaps_per_s": n / (t3 - t2)}}
    rec["parity_vs_checker"] = bool(parity)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
