#!/usr/bin/env python3
"""Batch ristretto255 / base-mode OPRF rates on one GPU.

    python tools/oprf_bench.py [--sizes 10,16,20] [--input 32] [--passes 3] [--min-ms 200] [--out profiles/oprf_bench.txt]

Per batch size n, alternated in one process over --passes passes:
    evaluate       circl_hip_oprf_evaluate, ONE key for the batch (stride 0): the server's operation
    evaluate/keys  the same with a key per item (stride 32)
    blind          circl_hip_oprf_blind, mode 0, inputs of --input bytes
    finalize       circl_hip_oprf_finalize
    full_evaluate  circl_hip_oprf_full_evaluate, mode 0, one key
    mult           circl_hip_ristretto255_scalar_mult on elements (no inversion): the bare constant-time multiplication
    mult_gen       the same on the generator: the fixed-base comb
    x25519         circl_hip_x25519_dev on n scalars and points: the ladder, the yardstick of a variable-base multiplication here
_dev rows: device events around at least --min-ms of back-to-back calls on resident tensors after a warm-up.  host rows: wall clock of
the host forms on numpy arrays through the ctypes binding (page-able memory, the staging pipeline, the list-to-blob packing of the
Python wrapper included, so they understate the C ABI).  Each figure: items per second from the mean of the passes, and the spread
(max / min - 1) of the passes.  finalize(evaluate(blind(x))) is checked to equal full_evaluate(x) at every size.  Writes the table to
--out with the command on its first line, and prints it.  Ed25519 verification, the other yardstick, is tools/ed25519_bench.py's to
measure in the same session."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circl_amd import device as cdev  # noqa: E402
from circl_amd import hostapi as api  # noqa: E402

ORDER = 2**252 + 27742317777372353535851937790883648493


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


def _wall_for(fn, min_ms):
    fn()
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        ms = (time.perf_counter() - t0) * 1e3
        if ms >= min_ms and reps >= 2:
            return ms / reps


def scalars(rng, n):
    """n scalars below the group order, not zero: 31 random bytes and a set low bit"""
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 0] |= 1
    a[:, 31] = 0
    return a


class Uniform(cdev.Ragged):
    """n items of `length` bytes each on the device, without building a list"""

    def __init__(self, blob, n, length):
        self.off_host = np.arange(n + 1, dtype=np.int64) * length
        self.blob = torch.from_numpy(blob).cuda()
        self.off = torch.from_numpy(self.off_host).cuda()


def bench(lg, in_len, passes, min_ms, rng, with_host):
    n = 1 << lg
    d = cdev.OprfDevice()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    blob = rng.integers(0, 256, n * in_len + 16, dtype=np.uint8)
    inputs_dev = Uniform(blob, n, in_len)
    blinds_h, keys_h = scalars(rng, n), scalars(rng, n)
    blinds, keys, key = t(blinds_h), t(keys_h), t(keys_h[:1])
    blinded, ok_b = d.blind(0, inputs_dev, blinds)
    evaluated, ok_e = d.evaluate(key, blinded)
    out, ok_f = d.finalize(inputs_dev, blinds, evaluated)
    full, ok_full = d.full_evaluate(0, key, inputs_dev, n)
    torch.cuda.synchronize()
    good = bool(ok_b.all().item() and ok_e.all().item() and ok_f.all().item() and ok_full.all().item() and (out == full).all().item())
    x_k, x_u = t(rng.integers(0, 256, (n, 32), dtype=np.uint8)), t(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    calls = {
        "evaluate": lambda: d.evaluate(key, blinded),
        "evaluate/keys": lambda: d.evaluate(keys, blinded),
        "blind": lambda: d.blind(0, inputs_dev, blinds),
        "finalize": lambda: d.finalize(inputs_dev, blinds, evaluated),
        "full_evaluate": lambda: d.full_evaluate(0, key, inputs_dev, n),
        "mult": lambda: d.scalar_mult(keys, blinded),
        "mult_gen": lambda: d.scalar_mult(keys),
        "x25519": lambda: cdev.x25519(x_k, x_u),
    }
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, fn in calls.items():
            ms[name].append(_timed_for(fn, min_ms))
    rows = {"dev": ms}
    if with_host:
        blinded_h, evaluated_h = blinded.cpu().numpy(), evaluated.cpu().numpy()
        key_h = keys_h[0].tobytes()
        items = [blob[i * in_len:(i + 1) * in_len].tobytes() for i in range(n)]
        host = {
            "evaluate": lambda: api.oprf_evaluate(key_h, blinded_h),
            "evaluate/keys": lambda: api.oprf_evaluate(keys_h, blinded_h),
            "blind": lambda: api.oprf_blind(0, items, blinds_h),
            "finalize": lambda: api.oprf_finalize(items, blinds_h, evaluated_h),
            "full_evaluate": lambda: api.oprf_full_evaluate(0, key_h, items),
            "mult": lambda: api.ristretto255_scalar_mult(keys_h, blinded_h),
            "mult_gen": lambda: api.ristretto255_scalar_mult(keys_h),
            "x25519": lambda: api.x25519(x_k.cpu().numpy(), x_u.cpu().numpy()),
        }
        hms = {name: [] for name in host}
        for _ in range(passes):
            for name, fn in host.items():
                hms[name].append(_wall_for(fn, min_ms))
        rows["host"] = hms
        good &= bool((api.oprf_full_evaluate(0, key_h, items)[0] == full.cpu().numpy()).all())
    return n, rows, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,16,20")
    ap.add_argument("--input", type=int, default=32)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oprf_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/oprf_bench.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9497)
    names = ["evaluate", "evaluate/keys", "blind", "finalize", "full_evaluate", "mult", "mult_gen", "x25519"]
    lines = ["python tools/oprf_bench.py " + " ".join(sys.argv[1:]),
             "%s; items per second (from the mean ms per call of %d passes) and spread = max / min - 1 of the passes; ristretto255-SHA512, mode 0, inputs of %d bytes" %
             (torch.cuda.get_device_name(0), a.passes, a.input),
             "%-5s %8s " % ("form", "n") + " ".join("%14s %6s" % (x, "spread") for x in names) + "  evaluate/x25519  checked"]
    for lg in [int(x) for x in a.sizes.split(",") if x]:
        n, rows, good = bench(lg, a.input, a.passes, a.min_ms, rng, not a.no_host)
        for form, ms in rows.items():
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: max(v) / min(v) - 1.0 for k, v in ms.items()}
            lines.append("%-5s %8d " % (form, n) + " ".join("%14.4g %5.1f%%" % (n / mean[x] * 1e3, 100 * spread[x]) for x in names) +
                         "  %15.3f  %s" % (mean["x25519"] / mean["evaluate"], "ok" if good else "MISMATCH"))
            print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
