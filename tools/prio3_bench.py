#!/usr/bin/env python3
"""Batch Prio3Count / Prio3Sum rates on one GPU (the _dev forms on resident inputs).

    python tools/prio3_bench.py [--lg 14,18] [--types count,255,65535,4294967295] [--shares 2] [--passes 3] [--min-ms 200]
                                [--out profiles/prio3_bench.txt]

Per batch size 2^lg and type (Count, or Sum with the given max_measurement): circl_hip_prio3_shard_dev, _prep_init_dev as the leader (on
the leader shares Shard made) and as helper 1 (on its seeds), _prep_finish_dev on the prep shares of both, in reports per second, and
_aggregate_dev in elements per second.  Random measurements, rand, nonces and verify key.  Device events around at least --min-ms of
back-to-back calls after a warm-up, over --passes passes.  Each figure: the rate from the mean of the passes, and the spread
(max / min - 1) of the passes; a second table has the mean microseconds per call, since a call that takes the same time at both batch
sizes is bound by the call itself (its launches and the wrapper's allocations), not by its kernels.  Every report of every shape must
prepare and be accepted (ok all 1), and the aggregate of the out shares must unshard to the sum of the measurements.

Writes the table to --out with the command on its first line, and prints it.  The static figures of the kernels (STATIC below) stand
beside the measured ones; they come from the compiler, not from a run."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circl_amd import _native as nat  # noqa: E402
from circl_amd import device as dev  # noqa: E402

STATIC = ("static figures (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; not measurements): shard / prep_init kernels: Count 94 / 96 "
          "VGPRs, Sum 90 / 100 VGPRs; no scratch, 10752 bytes of LDS per wavefront (the sponge's block buffer), occupancy 4 in all four; prep_finish 26 / 22 VGPRs, "
          "aggregate 14 VGPRs, occupancy 8.")
OPS = ("shard", "prep_init leader", "prep_init helper", "prep_finish", "aggregate")


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _timed_for(fn, min_ms):
    once = _timed(fn, 2)
    return _timed(fn, max(3, int(min_ms / max(once, 1e-3)) + 1))


def bench(kind, mx, shares, n, passes, min_ms, rng):
    """-> ({op: [ms per pass]}, everything checked)"""
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d = dev.Prio3Device(kind, mx, shares, b"prio3 bench: a task id of 40 bytes......")
    meas_h = rng.integers(0, min(mx, 2**62) + 1 if kind == 2 else 2, n, dtype=np.int64)
    meas, rand = t(meas_h), t(rng.integers(0, 256, (n, 32 * shares), dtype=np.uint8))
    nonces, vk = t(rng.integers(0, 256, (n, 16), dtype=np.uint8)), t(rng.integers(0, 256, 32, dtype=np.uint8))
    leader, ok = d.shard(meas, rand)
    good = bool(ok.all().item())
    seeds = [rand[:, 32 * j:32 * j + 32].contiguous() for j in range(shares - 1)]
    preps = torch.empty((n, shares, d.prep_share_size), dtype=torch.uint8, device="cuda")
    aggs = []
    for j in range(shares):
        p, out, ok = d.prep_init(j, vk, nonces, leader if j == 0 else seeds[j - 1])
        good &= bool(ok.all().item())
        preps[:, j] = p
        aggs.append(d.aggregate(torch.zeros(8, dtype=torch.uint8, device="cuda"), out).cpu().numpy().tobytes())
    good &= bool(d.prep_finish(preps).all().item())
    res = C.c_uint64(0)
    a = np.frombuffer(b"".join(aggs), np.uint8).copy()
    rc = nat.lib().circl_hip_prio3_unshard(*d.task, a.ctypes.data_as(C.c_void_p), n, C.byref(res))
    good &= rc != 0 if kind == 2 and n * mx >= 2**64 - 2**32 + 1 else rc == 0 and res.value == int(meas_h.sum())
    acc = torch.zeros(8, dtype=torch.uint8, device="cuda")
    kinds = {"shard": lambda: d.shard(meas, rand), "prep_init leader": lambda: d.prep_init(0, vk, nonces, leader),
             "prep_init helper": lambda: d.prep_init(1, vk, nonces, seeds[0]), "prep_finish": lambda: d.prep_finish(preps),
             "aggregate": lambda: d.aggregate(acc, out)}
    ms = {k: [] for k in kinds}
    for _ in range(passes):
        for k, fn in kinds.items():
            ms[k].append(_timed_for(fn, min_ms))
    return ms, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", default="14,18")
    ap.add_argument("--types", default="count,255,65535,4294967295")
    ap.add_argument("--shares", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prio3_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/prio3_bench.py needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(64)
    lines = ["python tools/prio3_bench.py " + " ".join(sys.argv[1:]),
             "%s; _dev forms, %d shares; reports (aggregate: elements) per second from the mean ms per call of %d passes, spread = max / min - 1 of the passes"
             % (torch.cuda.get_device_name(0), a.shares, a.passes), STATIC,
             "%-22s %8s " % ("type", "n") + " ".join("%16s %6s" % (op + " /s", "spread") for op in OPS)]
    worst, per_call = 0.0, ["microseconds per call (mean of the passes); where a call takes the same time at both batch sizes the rate above is the call's, not the kernel's",
                            "%-22s %8s " % ("type", "n") + " ".join("%16s" % op for op in OPS)]
    for ty in a.types.split(","):
        kind, mx = (1, 0) if ty == "count" else (2, int(ty))
        for lg in (int(x) for x in a.lg.split(",")):
            n = 1 << lg
            ms, good = bench(kind, mx, a.shares, n, a.passes, a.min_ms, rng)
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: max(v) / min(v) - 1.0 for k, v in ms.items()}
            worst = max(worst, max(spread.values()))
            lines.append("%-22s %8d " % ("Count" if kind == 1 else "Sum max %d" % mx, n) +
                         " ".join("%16.4g %5.1f%%" % (n / mean[op] * 1e3, 100 * spread[op]) for op in OPS) + ("  ok" if good else "  MISMATCH"))
            per_call.append("%-22s %8d " % ("Count" if kind == 1 else "Sum max %d" % mx, n) + " ".join("%16.1f" % (1e3 * mean[op]) for op in OPS))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    lines += per_call
    lines.append("largest spread of any figure above: %.1f%%" % (100 * worst))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4] + lines[-1:]))


if __name__ == "__main__":
    main()
