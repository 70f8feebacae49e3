#!/usr/bin/env python3
"""Batch DLEQ prove / verify rates on P-256 and P-384 on one GPU, device-resident.

    python tools/dleq_nistp_bench.py [--curves 256,384] [--elems 20] [--requests 1,8,64,65535] [--passes 3] [--min-ms 200]
                                     [--out profiles/dleq_nistp_bench.txt]

Per curve and request size s: 2^elems // s requests of s element pairs each under one key, through circl_hip_nistp_dleq_prove_dev /
_verify_dev on resident tensors with a workspace allocated once; device events around at least --min-ms of back-to-back calls after a
warm-up, alternated over --passes passes with `mult`: circl_hip_nistp_scalar_mult_dev on as many elements, the bare constant-time
multiplication, in the same process.  Columns: elements per second (from the mean of the passes), the spread (max / min - 1), the call's
time in units of one bare multiplication per element (the structure predicts about 1 for prove and 2 for verify, plus 3 and 4 per
request), and the split of one profiled call between the two kernels.  Every proof is verified (all 1) and, with one flipped bit per
proof, refused (all 0).  Writes the table to --out with the command on its first line, and prints it."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circl_amd import _native as nat  # noqa: E402
from circl_amd import device as cdev  # noqa: E402
from oprf_bench import _timed_for  # noqa: E402


def scalars(rng, n, ns):
    """n big-endian scalars below the group order, not zero: a cleared top byte and a set low bit"""
    a = rng.integers(0, 256, (n, ns), dtype=np.uint8)
    a[:, 0] = 0
    a[:, ns - 1] |= 1
    return a


def bench(curve, n_total, size, passes, min_ms, rng):
    lib, d = nat.lib(), cdev.NistpOprfDevice(curve)
    ns, ne = d.Ns, d.Ne
    n_req = max(1, n_total // size)
    n = n_req * size
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    key, r = t(scalars(rng, 1, ns)), t(scalars(rng, n_req, ns))
    B, ok_b = d.scalar_mult(t(scalars(rng, n, ns)))
    kB, ok_k = d.scalar_mult(key, B)
    kA, _ = d.scalar_mult(key, n=1)
    off = t(np.arange(n_req + 1, dtype=np.int64) * size)
    wsb = lib.circl_hip_nistp_dleq_workspace_size(curve, n_req, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    proofs, ok, verdict = (torch.empty(s, dtype=torch.uint8, device="cuda") for s in ((n_req, 2 * ns), (n_req,), (n_req,)))
    ctx_bytes = d._ctx(1)
    ctx = np.frombuffer(ctx_bytes + b"\0", np.uint8)
    tail = (ctx.ctypes.data_as(C.c_void_p), len(ctx_bytes), 1)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda x: x.data_ptr()  # noqa: E731

    def prove():
        nat.check(lib.circl_hip_nistp_dleq_prove_dev(curve, p(key), 0, p(kA), 0, p(B), p(kB), p(off), p(r), *tail, p(proofs), p(ok), n_req, n, p(ws), wsb, st()),
                  "prove")

    def verify(pr=proofs):
        nat.check(lib.circl_hip_nistp_dleq_verify_dev(curve, p(kA), 0, p(B), p(kB), p(off), p(pr), *tail, p(verdict), n_req, n, p(ws), wsb, st()), "verify")

    prove()
    verify()
    torch.cuda.synchronize()
    good = bool(ok_b.all().item() and ok_k.all().item() and ok.all().item() and verdict.all().item())
    bad = proofs.clone()
    bad[:, ns + 1] ^= 2
    verify(bad)
    torch.cuda.synchronize()
    good &= not bool(verdict.any().item())
    calls = {"prove": prove, "verify": verify, "mult": lambda: d.scalar_mult(key, B)}
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, fn in calls.items():
            ms[name].append(_timed_for(fn, min_ms))
    split = {}
    for name, fn in (("prove", prove), ("verify", verify)):
        lib.circl_hip_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        part = []
        for kid in (cdev.KERNELS["dleq_composite"], cdev.KERNELS["dleq_finish"]):     # (the NIST launches report under the same ids)
            tot, cnt = C.c_double(0), C.c_uint64(0)
            lib.circl_hip_profile_read(kid, C.byref(tot), C.byref(cnt))
            part.append(tot.value)
        lib.circl_hip_profile_enable(0)
        split[name] = part
    return n_req, n, ms, split, good, wsb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="256,384")
    ap.add_argument("--elems", type=int, default=20)
    ap.add_argument("--requests", default="1,8,64,65535")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dleq_nistp_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/dleq_nistp_bench.py needs a GPU: nothing is measured without one")
    rng = np.random.default_rng(2292)
    lines = ["python tools/dleq_nistp_bench.py " + " ".join(sys.argv[1:]),
             "%s; device-resident, one key per call; elements per second from the mean ms per call of %d passes, spread = max / min - 1; "
             "mults/elem = the call's time over the bare nistp_scalar_mult time per element (predicted: ~1 prove, ~2 verify, plus 3 / 4 per request); "
             "composite+finish = the two kernels' ms in one profiled call" % (torch.cuda.get_device_name(0), a.passes),
             "%6s %8s %9s %9s  %12s %6s %10s %16s  %12s %6s %10s %16s  %12s %6s  %10s  %s" %
             ("curve", "req size", "requests", "elements", "prove el/s", "spread", "mults/elem", "composite+finish", "verify el/s", "spread", "mults/elem",
              "composite+finish", "mult el/s", "spread", "workspace", "checked")]
    for curve in [int(x) for x in a.curves.split(",") if x]:
        for size in [int(x) for x in a.requests.split(",") if x]:
            n_req, n, ms, split, good, wsb = bench(curve, 1 << a.elems, size, a.passes, a.min_ms, rng)
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            spread = {k: max(v) / min(v) - 1.0 for k, v in ms.items()}
            cols = []
            for name in ("prove", "verify"):
                cols.append("%12.4g %5.1f%% %10.2f %16s" % (n / mean[name] * 1e3, 100 * spread[name], mean[name] / mean["mult"], "%.2f+%.2f" % tuple(split[name])))
            lines.append("%6s %8d %9d %9d  %s  %s  %12.4g %5.1f%%  %10d  %s" % ("P-%d" % curve, size, n_req, n, cols[0], cols[1], n / mean["mult"] * 1e3,
                                                                              100 * spread["mult"], wsb, "ok" if good else "MISMATCH"))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
