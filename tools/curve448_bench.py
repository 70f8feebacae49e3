#!/usr/bin/env python3
"""Batch X448 / Ed448 rates on one GPU: prints ONE JSON record.

    python tools/curve448_bench.py [--sizes 10,14,18,20] [--reps 3] [--host-sizes 10,14,18] [--route-sizes 14,18] [--hybrid-size 16]

device-resident: the _dev entry points on torch buffers, one key per item, 64-byte messages, empty contexts, timed with CUDA
events around `reps` launches after a warm-up; x25519_shared / x25519_keygen: circl_hip_x25519_dev at the same sizes in the same
process, so that the X448 : X25519 ratio is on file; host: the host-buffer entry points on numpy arrays (wall clock, including
the Python binding's per-item list building, so they understate the C ABI); n = 1 latency of the host forms; parity: a sample of
every device batch checked against the checker of tests/curve448.py.
x448_keygen_routes: circl_hip_x448_dev KeyGen by the ladder and by the Ed448 comb (CIRCL_HIP_X448_KEYGEN, read at every call),
alternated twice in this one process at each of --route-sizes, every figure from device events around at least 300 ms of
back-to-back calls on inputs resident in HBM; "comb_faster" is true for a size when the comb's slowest pass beats the ladder's
fastest.  hybrids: KeyGen / Encaps / Decaps of Kyber768-X448, Kyber1024-X448 and, for scale, Kyber768-X25519 through the _dev entry
points at 2^--hybrid-size, timed the same way (with the default KeyGen route)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import curve448 as ref  # noqa: E402
from circl_amd import _native as nat  # noqa: E402
from circl_amd import hostapi  # noqa: E402


def _timed(fn, name, reps):
    nat.check(fn(), name)  # warm-up (and the inputs of the next operation)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        nat.check(fn(), name)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _timed_for(fn, name, min_ms=300.0):
    """ms per call from device events around at least `min_ms` of back-to-back calls"""
    once = _timed(fn, name, 2)
    reps = max(3, int(min_ms / max(once, 1e-3)) + 1)
    return _timed(fn, name, reps), reps


def keygen_routes(L, dev, lgs, rng):
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rec = {}
    for lg in lgs:
        n = 1 << lg
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        kh = rng.integers(0, 256, (n, 56), dtype=np.uint8)
        k = torch.from_numpy(kh).to(dev)
        pubs = {r: torch.empty((n, 56), dtype=torch.uint8, device=dev) for r in ("ladder", "comb")}
        row = {"ladder_per_s": [], "comb_per_s": [], "ladder_ms": [], "comb_ms": [], "reps": []}
        for _ in range(2):
            for route in ("ladder", "comb"):
                os.environ["CIRCL_HIP_X448_KEYGEN"] = route
                ms, reps = _timed_for(lambda: L.circl_hip_x448_dev(vp(k), None, vp(pubs[route]), None, n, st), "x448_keygen " + route)
                row[route + "_per_s"].append(n / (ms / 1e3))
                row[route + "_ms"].append(ms)
                row["reps"].append(reps)
        os.environ.pop("CIRCL_HIP_X448_KEYGEN", None)
        row["same_bytes"] = bool((pubs["ladder"] == pubs["comb"]).all().item())
        ph = pubs["comb"].cpu().numpy()
        row["parity_vs_checker"] = all(bytes(ph[i]) == ref.x448(bytes(kh[i]))[0] for i in rng.choice(n, 8, replace=False))
        row["comb_to_ladder"] = min(row["comb_per_s"]) / max(row["ladder_per_s"])
        row["comb_faster"] = row["comb_to_ladder"] > 1.0
        rec["2^%d" % lg] = row
        del k, pubs
    rec["comb_faster_at_every_size"] = bool(rec) and all(r["comb_faster"] for r in rec.values())
    return rec


def hybrids(dev, lg, rng):
    from circl_amd import device as dv
    n = 1 << lg
    rec = {"n": n}
    for name, scheme in (("Kyber768-X448", dv.KYBER768_X448), ("Kyber1024-X448", dv.KYBER1024_X448), ("Kyber768-X25519", dv.KYBER768_X25519)):
        H = dv.HybridDevice(scheme, n)
        seeds = torch.from_numpy(rng.integers(0, 256, (n, H.S["seed"]), dtype=np.uint8)).to(dev)
        es = torch.from_numpy(rng.integers(0, 256, (n, H.S["eseed"]), dtype=np.uint8)).to(dev)
        row = {}
        for op, fn in (("keygen", lambda: (H.keygen(seeds), 0)[1]), ("encaps", lambda: (H.encaps(H.pk, es), 0)[1]),
                       ("decaps", lambda: (H.decaps(H.sk, H.ct), 0)[1])):
            ms, reps = _timed_for(fn, name + " " + op)
            row[op + "_per_s"], row[op + "_ms"], row[op + "_reps"] = n / (ms / 1e3), ms, reps
        row["round_trip_ok"] = bool((H.ss == H.ss2).all().item()) and not bool(H.status.any().item())
        rec[name] = row
        del H, seeds, es
        torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,18,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sizes", default="10,14,18")
    ap.add_argument("--route-sizes", default="14,18")
    ap.add_argument("--hybrid-size", type=int, default=16)
    a = ap.parse_args()
    L = nat.lib()
    dev = torch.device("cuda:0")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rec = {"tool": "tools/curve448_bench.py", "device": torch.cuda.get_device_name(0), "msg_bytes": 64, "ctx_bytes": 0, "device_resident": {}, "host": {}}
    parity = True
    rng = np.random.default_rng(1)
    for lg in [int(x) for x in a.sizes.split(",") if x]:
        n = 1 << lg
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        row = {}
        # X448 and, beside it, X25519
        kh, uh = rng.integers(0, 256, (n, 56), dtype=np.uint8), rng.integers(0, 256, (n, 56), dtype=np.uint8)
        k, u = torch.from_numpy(kh).to(dev), torch.from_numpy(uh).to(dev)
        out = torch.empty((n, 56), dtype=torch.uint8, device=dev)
        pub = torch.empty((n, 56), dtype=torch.uint8, device=dev)
        okx = torch.empty(n, dtype=torch.uint8, device=dev)
        k25, u25 = k[:, :32].contiguous(), u[:, :32].contiguous()
        o25 = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        xops = {"x448_shared": lambda: L.circl_hip_x448_dev(vp(k), vp(u), vp(out), vp(okx), n, st),
                "x448_keygen": lambda: L.circl_hip_x448_dev(vp(k), None, vp(pub), None, n, st),
                "x25519_shared": lambda: L.circl_hip_x25519_dev(vp(k25), vp(u25), vp(o25), None, n, st),
                "x25519_keygen": lambda: L.circl_hip_x25519_dev(vp(k25), None, vp(o25), None, n, st)}
        for name, fn in xops.items():
            ms = _timed(fn, name, a.reps)
            row[name + "_per_s"], row[name + "_ms"] = n / (ms / 1e3), ms
        row["x448_to_x25519_shared"] = row["x448_shared_per_s"] / row["x25519_shared_per_s"]
        oh, ph = out.cpu().numpy(), pub.cpu().numpy()
        for i in rng.choice(n, min(n, 8), replace=False):
            parity &= bytes(oh[i]) == ref.x448(bytes(kh[i]), bytes(uh[i]))[0]
            parity &= bytes(ph[i]) == ref.x448(bytes(kh[i]))[0]
        del k, u, out, pub, okx, k25, u25, o25
        # Ed448
        seeds = torch.from_numpy(rng.integers(0, 256, (n, 57), dtype=np.uint8)).to(dev)
        msg = rng.integers(0, 256, (n, 64), dtype=np.uint8)
        d_mb = torch.from_numpy(msg.reshape(-1)).to(dev)
        d_mo = torch.arange(0, 64 * (n + 1), 64, dtype=torch.int64, device=dev)
        pk = torch.empty((n, 57), dtype=torch.uint8, device=dev)
        sk = torch.empty((n, 114), dtype=torch.uint8, device=dev)
        sig = torch.empty((n, 114), dtype=torch.uint8, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        wsb = L.circl_hip_ed448_workspace_size(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        ops = {"keygen": lambda: L.circl_hip_ed448_keygen_dev(vp(seeds), vp(pk), vp(sk), n, vp(ws), wsb, st),
               "sign": lambda: L.circl_hip_ed448_sign_dev(vp(sk), vp(d_mb), vp(d_mo), None, None, vp(sig), n, vp(ws), wsb, st),
               "verify": lambda: L.circl_hip_ed448_verify_dev(vp(pk), vp(sig), vp(d_mb), vp(d_mo), None, None, vp(ok), n, vp(ws), wsb, st)}
        for name, fn in ops.items():
            ms = _timed(fn, name, a.reps)
            row["ed448_" + name + "_per_s"], row["ed448_" + name + "_ms"] = n / (ms / 1e3), ms
        parity &= bool(ok.cpu().numpy().all())
        pkh, skh, sgh = pk.cpu().numpy(), sk.cpu().numpy(), sig.cpu().numpy()
        for i in rng.choice(n, min(n, 8), replace=False):
            parity &= bytes(pkh[i]) == ref.public(bytes(skh[i][:57]))
            parity &= bytes(sgh[i]) == ref.sign(bytes(skh[i]), msg[i].tobytes())
        rec["device_resident"]["2^%d" % lg] = row
        del seeds, d_mb, d_mo, pk, sk, sig, ok, ws
        torch.cuda.empty_cache()
    for lg in [int(x) for x in a.host_sizes.split(",") if x]:
        n = 1 << lg
        seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
        msgs = [bytes(r) for r in rng.integers(0, 256, (n, 64), dtype=np.uint8)]
        k, u = rng.integers(0, 256, (n, 56), dtype=np.uint8), rng.integers(0, 256, (n, 56), dtype=np.uint8)
        hostapi.ed448_keygen(seeds[:64])
        hostapi.x448(k[:64], u[:64])
        t = time.perf_counter(); pk, sk = hostapi.ed448_keygen(seeds); t1 = time.perf_counter()
        sig = hostapi.ed448_sign(sk, msgs); t2 = time.perf_counter()
        ok = hostapi.ed448_verify(pk, sig, msgs); t3 = time.perf_counter()
        hostapi.x448(k, u); t4 = time.perf_counter()
        parity &= bool(ok.all())
        rec["host"]["2^%d" % lg] = {"ed448_keygen_per_s": n / (t1 - t), "ed448_sign_per_s": n / (t2 - t1), "ed448_verify_per_s": n / (t3 - t2),
                                    "x448_shared_per_s": n / (t4 - t3)}
    seeds = rng.integers(0, 256, (1, 57), dtype=np.uint8)
    k1, u1 = rng.integers(0, 256, (1, 56), dtype=np.uint8), rng.integers(0, 256, (1, 56), dtype=np.uint8)
    lat = {}
    for _ in range(2):
        t = time.perf_counter(); pk, sk = hostapi.ed448_keygen(seeds); t1 = time.perf_counter()
        sig = hostapi.ed448_sign(sk, [b"m" * 64]); t2 = time.perf_counter()
        ok = hostapi.ed448_verify(pk, sig, [b"m" * 64]); t3 = time.perf_counter()
        hostapi.x448(k1, u1); t4 = time.perf_counter()
        lat = {"ed448_keygen_ms": (t1 - t) * 1e3, "ed448_sign_ms": (t2 - t1) * 1e3, "ed448_verify_ms": (t3 - t2) * 1e3, "x448_shared_ms": (t4 - t3) * 1e3}
    rec["n1_latency"] = lat
    rec["x448_keygen_routes"] = keygen_routes(L, dev, [int(x) for x in a.route_sizes.split(",") if x], rng)
    if a.hybrid_size > 0:
        rec["hybrids"] = hybrids(dev, a.hybrid_size, rng)
    rec["parity_vs_checker"] = bool(parity)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
