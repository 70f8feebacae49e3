#!/usr/bin/env python3
"""Batch Ed25519 rates on one GPU: prints ONE JSON record.

    python tools/ed25519_bench.py [--sizes 10,14,18,20] [--reps 3]

device-resident: the _dev entry points on torch buffers, one key per item, 64-byte messages, timed with CUDA events around
`reps` launches after a warm-up; host: the host-buffer entry points on numpy arrays (wall clock, including the Python binding's
per-item list building, so they understate the C ABI); n = 1 latency of the host
forms; parity: a sample of every device batch checked against the RFC 8032 checker of tests/ed25519.py; cpu_openssl: the
output of `openssl speed -multi 16 ed25519` when the box has an openssl binary (labelled, not compared)."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ed25519 as ref  # noqa: E402
from circl_amd import _native as nat  # noqa: E402
from circl_amd import hostapi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,18,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sizes", default="10,14,18,20")
    a = ap.parse_args()
    L = nat.lib()
    dev = torch.device("cuda:0")
    vp = lambda t: C.c_void_p(t.data_ptr())
    rec = {"tool": "tools/ed25519_bench.py", "device": torch.cuda.get_device_name(0), "msg_bytes": 64, "device_resident": {}, "host": {}}
    parity = True
    rng = np.random.default_rng(1)
    for lg in [int(x) for x in a.sizes.split(",")]:
        n = 1 << lg
        seeds = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
        msg = rng.integers(0, 256, (n, 64), dtype=np.uint8)
        d_mb = torch.from_numpy(msg.reshape(-1)).to(dev)
        d_mo = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device=dev)
        pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        sk = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        wsb = L.circl_hip_ed25519_workspace_size(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ops = {"keygen": lambda: L.circl_hip_ed25519_keygen_dev(vp(seeds), vp(pk), vp(sk), n, vp(ws), wsb, st),
               "sign": lambda: L.circl_hip_ed25519_sign_dev(vp(sk), vp(d_mb), vp(d_mo), vp(sig), n, vp(ws), wsb, st),
               "verify": lambda: L.circl_hip_ed25519_verify_dev(vp(pk), vp(sig), vp(d_mb), vp(d_mo), vp(ok), n, vp(ws), wsb, st)}
        row = {}
        for name, fn in ops.items():
            nat.check(fn(), name)  # warm-up (and the inputs of the next operation)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                nat.check(fn(), name)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            row[name + "_per_s"] = n / (ms / 1e3)
            row[name + "_ms"] = ms
        okh = ok.cpu().numpy()
        pkh, skh, sgh = pk.cpu().numpy(), sk.cpu().numpy(), sig.cpu().numpy()
        idx = rng.choice(n, min(n, 16), replace=False)
        parity &= bool(okh.all())
        for i in idx:
            parity &= bytes(pkh[i]) == ref.public(bytes(skh[i][:32]))
            parity &= bytes(sgh[i]) == ref.sign(bytes(skh[i]), msg[i].tobytes())
        rec["device_resident"]["2^%d" % lg] = row
        del seeds, d_mb, d_mo, pk, sk, sig, ok, ws
        torch.cuda.empty_cache()
    for lg in [int(x) for x in a.host_sizes.split(",") if x]:
        n = 1 << lg
        seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        msgs = [bytes(r) for r in rng.integers(0, 256, (n, 64), dtype=np.uint8)]
        hostapi.ed25519_keygen(seeds[:64])
        t = time.perf_counter(); pk, sk = hostapi.ed25519_keygen(seeds); t1 = time.perf_counter()
        sig = hostapi.ed25519_sign(sk, msgs); t2 = time.perf_counter()
        ok = hostapi.ed25519_verify(pk, sig, msgs); t3 = time.perf_counter()
        parity &= bool(ok.all())
        rec["host"]["2^%d" % lg] = {"keygen_per_s": n / (t1 - t), "sign_per_s": n / (t2 - t1), "verify_per_s": n / (t3 - t2)}
    seeds = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    lat = {}
    for _ in range(2):
        t = time.perf_counter(); pk, sk = hostapi.ed25519_keygen(seeds); t1 = time.perf_counter()
        sig = hostapi.ed25519_sign(sk, [b"m" * 64]); t2 = time.perf_counter()
        ok = hostapi.ed25519_verify(pk, sig, [b"m" * 64]); t3 = time.perf_counter()
        lat = {"keygen_ms": (t1 - t) * 1e3, "sign_ms": (t2 - t1) * 1e3, "verify_ms": (t3 - t2) * 1e3}
    rec["n1_latency"] = lat
    rec["parity_vs_checker"] = bool(parity)
    if shutil.which("openssl"):
        try:
            out = subprocess.run(["openssl", "speed", "-seconds", "2", "-multi", "16", "ed25519"], capture_output=True, text=True, timeout=120).stdout
            rec["cpu_openssl_speed_multi16_ed25519"] = [l for l in out.splitlines() if "ed25519" in l.lower()][-2:]
        except (OSError, subprocess.SubprocessError) as e:
            rec["cpu_openssl_speed_multi16_ed25519"] = "failed: %s" % e
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
