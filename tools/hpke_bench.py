#!/usr/bin/env python3
"""Batch HPKE DHKEM rates (X25519 / HKDF-SHA256 and X448 / HKDF-SHA512) on one GPU: prints ONE JSON record.

    python tools/hpke_bench.py [--sizes 10,14,16,18] [--kems 0x20,0x21] [--passes 2] [--min-ms 300]

The _dev forms on inputs resident in HBM; every figure is milliseconds per call from device events around at least --min-ms of
back-to-back calls after a warm-up.  The yardstick is not the code under test: it is circl_hip_x25519_dev / circl_hip_x448_dev KeyGen
and Shared at the same n, in the same process, alternated with the fused calls over --passes passes.  A fused call is expected to
take at most (the sum of the scalar multiplications it contains) x (1 + h + s):
    derive_keypair: KeyGen            encap: KeyGen + Shared          decap (pkR NULL): KeyGen + Shared
    auth_encap (pkS NULL): 2 KeyGen + 2 Shared                         auth_decap (pkR NULL): KeyGen + 2 Shared
h = the share of hash-and-glue instructions in the kernel (H below), s = the spread (max / min - 1) of the yardstick sum over the
passes of this run.  "meets" is fused_ms (slowest pass) <= yardstick sum (mean over the passes) x (1 + h + s).
parity: a sample of every batch against the checker tests/hpke_dhkem.py."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpke_dhkem as ref  # noqa: E402
from circl_amd import _native as nat  # noqa: E402

# h: executed hash-and-glue instructions of the kernel / all executed instructions, counted from the -save-temps assembly of
# api_hpke.hip (the kernel's own body with its SHA loops at their trip counts, against the out-of-line comb and ladder with theirs)
H = {0x20: {"derive_keypair": 0.177, "encap": 0.108, "decap": 0.060, "auth_encap": 0.064, "auth_decap": 0.043},
     0x21: {"derive_keypair": 0.113, "encap": 0.069, "decap": 0.036, "auth_encap": 0.037, "auth_decap": 0.023}}
MULTS = {"derive_keypair": (1, 0), "encap": (1, 1), "decap": (1, 1), "auth_encap": (2, 2), "auth_decap": (1, 2)}  # (KeyGen, Shared)


def _timed(fn, name, reps):
    nat.check(fn(), name)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        nat.check(fn(), name)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _timed_for(fn, name, min_ms):
    once = _timed(fn, name, 2)
    return _timed(fn, name, max(3, int(min_ms / max(once, 1e-3)) + 1))


def bench(L, kem, lg, passes, min_ms, rng):
    k = ref.Kem(kem)
    n, N, S = 1 << lg, k.N, k.Nh
    dev = torch.device("cuda:0")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rnd = lambda: rng.integers(0, 256, (n, N), dtype=np.uint8)  # noqa: E731
    host = {name: rnd() for name in ("ikmR", "ikmS", "ikmE")}
    t = {name: torch.from_numpy(a).to(dev) for name, a in host.items()}
    for name in ("skR", "pkR", "skS", "pkS", "enc", "aenc", "tmp"):
        t[name] = torch.empty((n, N), dtype=torch.uint8, device=dev)
    for name in ("ss", "ss2", "ass", "ass2"):
        t[name] = torch.empty((n, S), dtype=torch.uint8, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    xdh = L.circl_hip_x25519_dev if kem == 0x20 else L.circl_hip_x448_dev
    nat.check(L.circl_hip_hpke_dhkem_derive_keypair_dev(kem, vp(t["ikmS"]), vp(t["skS"]), vp(t["pkS"]), n, st), "derive S")
    calls = {
        "keygen": lambda: xdh(vp(t["skS"]), None, vp(t["tmp"]), None, n, st),
        "shared": lambda: xdh(vp(t["skS"]), vp(t["pkR"]), vp(t["tmp"]), vp(ok), n, st),
        "derive_keypair": lambda: L.circl_hip_hpke_dhkem_derive_keypair_dev(kem, vp(t["ikmR"]), vp(t["skR"]), vp(t["pkR"]), n, st),
        "encap": lambda: L.circl_hip_hpke_dhkem_encap_dev(kem, vp(t["pkR"]), vp(t["ikmE"]), vp(t["enc"]), vp(t["ss"]), vp(ok), n, st),
        "decap": lambda: L.circl_hip_hpke_dhkem_decap_dev(kem, vp(t["skR"]), None, vp(t["enc"]), vp(t["ss2"]), vp(ok), n, st),
        "auth_encap": lambda: L.circl_hip_hpke_dhkem_auth_encap_dev(kem, vp(t["pkR"]), vp(t["skS"]), None, vp(t["ikmE"]), vp(t["aenc"]), vp(t["ass"]),
                                                                    vp(ok), n, st),
        "auth_decap": lambda: L.circl_hip_hpke_dhkem_auth_decap_dev(kem, vp(t["skR"]), None, vp(t["aenc"]), vp(t["pkS"]), vp(t["ass2"]), vp(ok), n, st),
    }
    order = ["derive_keypair", "keygen", "shared", "encap", "decap", "auth_encap", "auth_decap"]  # derive first: it makes skR / pkR
    ms = {name: [] for name in order}
    for _ in range(passes):
        for name in order:
            ms[name].append(_timed_for(calls[name], name, min_ms))
    row = {"n": n, "keygen_ms": ms["keygen"], "shared_ms": ms["shared"]}
    meets = True
    for op, (nk, ns) in MULTS.items():
        sums = [nk * a + ns * b for a, b in zip(ms["keygen"], ms["shared"])]
        s = max(sums) / min(sums) - 1.0
        yard = sum(sums) / len(sums)
        fused = max(ms[op])
        row[op] = {"ms": ms[op], "per_s": n / (min(ms[op]) / 1e3), "yardstick_ms": yard, "ratio": fused / yard, "h": H[kem][op], "s": s,
                   "meets": fused <= yard * (1.0 + H[kem][op] + s)}
        meets &= row[op]["meets"]
    row["meets"] = meets
    # parity of a sample against the checker, and the round trips of the whole batch
    g = {name: t[name].cpu().numpy() for name in ("skR", "pkR", "skS", "pkS", "enc", "ss", "aenc", "ass")}
    par = bool((t["ss"] == t["ss2"]).all().item()) and bool((t["ass"] == t["ass2"]).all().item())
    for i in rng.choice(n, min(n, 4), replace=False):
        par &= k.derive_keypair(bytes(host["ikmR"][i])) == (bytes(g["skR"][i]), bytes(g["pkR"][i]))
        par &= k.encap(bytes(g["pkR"][i]), bytes(host["ikmE"][i])) == (bytes(g["enc"][i]), bytes(g["ss"][i]))
        par &= k.auth_encap(bytes(g["pkR"][i]), bytes(g["skS"][i]), bytes(host["ikmE"][i])) == (bytes(g["aenc"][i]), bytes(g["ass"][i]))
    row["parity_vs_checker"] = bool(par)
    del t
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16,18")
    ap.add_argument("--kems", default="0x20,0x21")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=300.0)
    a = ap.parse_args()
    L = nat.lib()
    rng = np.random.default_rng(9180)
    rec = {"tool": "tools/hpke_bench.py", "device": torch.cuda.get_device_name(0), "passes": a.passes, "min_ms": a.min_ms}
    for kem in [int(x, 0) for x in a.kems.split(",") if x]:
        rec["0x%02x" % kem] = {"2^%d" % lg: bench(L, kem, lg, a.passes, a.min_ms, rng) for lg in [int(x) for x in a.sizes.split(",") if x]}
    rec["meets_everywhere"] = all(r["meets"] for k, v in rec.items() if k.startswith("0x") for r in v.values())
    rec["parity_vs_checker"] = all(r["parity_vs_checker"] for k, v in rec.items() if k.startswith("0x") for r in v.values())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
