#!/usr/bin/env python3
"""Batch P-256 / P-384 base-mode OPRF rates on one GPU, with the ristretto255 evaluate in the same process for scale.

    python tools/oprf_nistp_bench.py [--sizes 16,20] [--input 32] [--passes 3] [--min-ms 200] [--out profiles/oprf_nistp_bench.txt]

Per curve and batch size n, alternated in one process over --passes passes, on resident tensors (the _dev forms):
    evaluate        circl_hip_oprf_nistp_evaluate_dev, ONE key for the batch (stride 0): the server's operation
    full_evaluate   circl_hip_oprf_nistp_full_evaluate_dev, mode 0, one key, inputs of --input bytes
    blind           circl_hip_oprf_nistp_blind_dev, mode 0
    r255 evaluate   circl_hip_oprf_evaluate_dev on n ristretto255 elements, one key: the yardstick
Device events around at least --min-ms of back-to-back calls after a warm-up call.  Each figure: items per second from the mean of the
passes, and the spread (max / min - 1) of the passes.  finalize(evaluate(blind(x))) is checked to equal full_evaluate(x) at every size.
Writes the table to --out with the command on its first line, and prints it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circl_amd import device as cdev  # noqa: E402


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
    once = _timed(fn, 1)
    return _timed(fn, max(2, int(min_ms / max(once, 1e-3)) + 1))


def scalars(rng, n, width, big_endian):
    """n scalars below either group order, not zero: the top byte cleared and the low bit set"""
    a = rng.integers(0, 256, (n, width), dtype=np.uint8)
    a[:, 0 if big_endian else width - 1] = 0
    a[:, width - 1 if big_endian else 0] |= 1
    return a


class Uniform(cdev.Ragged):
    """n items of `length` bytes each on the device, without building a list"""

    def __init__(self, blob, n, length):
        self.off_host = np.arange(n + 1, dtype=np.int64) * length
        self.blob = torch.from_numpy(blob).cuda()
        self.off = torch.from_numpy(self.off_host).cuda()


def bench(lg, in_len, passes, min_ms, rng):
    n = 1 << lg
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    inputs = Uniform(rng.integers(0, 256, n * in_len + 16, dtype=np.uint8), n, in_len)
    calls, good = {}, True
    for curve in (256, 384):
        d = cdev.NistpOprfDevice(curve)
        blinds, key = t(scalars(rng, n, d.Ns, True)), t(scalars(rng, 1, d.Ns, True))
        blinded, ok_b = d.blind(0, inputs, blinds)
        evaluated, ok_e = d.evaluate(key, blinded)
        out, ok_f = d.finalize(inputs, blinds, evaluated)
        full, ok_full = d.full_evaluate(0, key, inputs, n)
        torch.cuda.synchronize()
        good &= bool(ok_b.all().item() and ok_e.all().item() and ok_f.all().item() and ok_full.all().item() and (out == full).all().item())
        calls["P-%d evaluate" % curve] = lambda d=d, key=key, blinded=blinded: d.evaluate(key, blinded)
        calls["P-%d full_evaluate" % curve] = lambda d=d, key=key: d.full_evaluate(0, key, inputs, n)
        calls["P-%d blind" % curve] = lambda d=d, blinds=blinds: d.blind(0, inputs, blinds)
    r = cdev.OprfDevice()
    r_blinded, _ = r.blind(0, inputs, t(scalars(rng, n, 32, False)))
    r_key = t(scalars(rng, 1, 32, False))
    calls["r255 evaluate"] = lambda: r.evaluate(r_key, r_blinded)
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, fn in calls.items():
            ms[name].append(_timed_for(fn, min_ms))
    return n, ms, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--input", type=int, default=32)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oprf_nistp_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/oprf_nistp_bench.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(9497)
    lines = ["python tools/oprf_nistp_bench.py " + " ".join(sys.argv[1:]),
             "%s; _dev forms, items per second (from the mean ms per call of %d passes) and spread = max / min - 1 of the passes; mode 0, one key, inputs of %d bytes" %
             (torch.cuda.get_device_name(0), a.passes, a.input)]
    for lg in [int(x) for x in a.sizes.split(",") if x]:
        n, ms, good = bench(lg, a.input, a.passes, a.min_ms, rng)
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        lines.append("n = %d  (finalize(evaluate(blind(x))) = full_evaluate(x): %s)" % (n, "ok" if good else "MISMATCH"))
        for name in ms:
            lines.append("  %-20s %12.4g items/s  %9.3f ms/call  spread %5.1f%%  r255 evaluate / this = %6.3f" %
                         (name, n / mean[name] * 1e3, mean[name], 100 * (max(ms[name]) / min(ms[name]) - 1.0), mean["r255 evaluate"] / mean[name]))
        print("\n".join(lines[-len(ms) - 1:]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
