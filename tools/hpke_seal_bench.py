#!/usr/bin/env python3
"""Single-shot HPKE Seal / Open against the bare DHKEM and against the two-call route, on one GPU.

    python tools/hpke_seal_bench.py [--sizes 10,14,18] [--pt 32,256,1024] [--passes 3] [--min-ms 300] [--out profiles/hpke_seal_bench.txt]

For X25519 / HKDF-SHA256 and X448 / HKDF-SHA512 with ChaCha20Poly1305 in base mode, on inputs resident in HBM (the _dev forms), at every
n and plaintext length (aad 8 bytes, info 20 bytes), alternated in one process over --passes passes:
    encap         circl_hip_hpke_dhkem_encap_dev            the yardstick of seal_single
    seal_single   circl_hip_hpke_seal_single_dev            one launch
    setup + seal  circl_hip_hpke_setup_sender_dev, then circl_hip_hpke_seal_dev on the context rows: two launches
    decap         circl_hip_hpke_dhkem_decap_dev            the yardstick of open_single (pkR given to both)
    open_single   circl_hip_hpke_open_single_dev
Every figure is milliseconds per call from device events around at least --min-ms of back-to-back calls after a warm-up.  Per row: the
mean over the passes, the spread (max / min - 1) of each, seal_single / encap, open_single / decap and (setup + seal) / seal_single.
The single-shot kernel is worth keeping where the last ratio exceeds 1 by more than the spreads.  The plaintexts are checked to come
back from open_single.  Writes the table to --out with the command on its first line, and prints it."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from circl_amd import _native as nat  # noqa: E402
from circl_amd import device as cdev  # noqa: E402

SUITES = [(0x20, 1, "X25519/SHA-256"), (0x21, 3, "X448/SHA-512")]


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


class Uniform:
    """n items of `length` bytes each as a device blob + offsets (what device.Ragged builds from a list, without the list)"""

    def __init__(self, rng, n, length):
        self.off_host = np.arange(n + 1, dtype=np.int64) * length
        self.blob = torch.from_numpy(rng.integers(0, 256, n * length + 16, dtype=np.uint8)).cuda()
        self.off = torch.from_numpy(self.off_host).cuda()

    def args(self):
        return self.blob.data_ptr(), self.off.data_ptr()


def bench(L, kem, kdf, lg, pt_len, passes, min_ms, rng):
    n = 1 << lg
    s = cdev.HpkeSuiteDevice(kem, kdf, 3)
    k = cdev.HpkeDhkemDevice(kem)
    rows = lambda: torch.from_numpy(rng.integers(0, 256, (n, s.N), dtype=np.uint8)).cuda()  # noqa: E731
    ikmR, ikmE = rows(), rows()
    skR, pkR = k.derive_keypair(ikmR)
    info, aad, pt = Uniform(rng, n, 20), Uniform(rng, n, 8), Uniform(rng, n, pt_len)
    enc, ss, ok = k.encap(pkR, ikmE)
    ss2 = torch.empty_like(ss)
    enc1, ct, ok1 = s.seal_single(0, pkR, ikmE, pt, aad, info)
    back, ok2 = s.open_single(0, skR, enc1, ct, pt, aad, info, pkR=pkR)
    torch.cuda.synchronize()
    good = bool(ok1.all().item() and ok2.all().item() and (back[:n * pt_len] == pt.blob[:n * pt_len]).all().item())
    enc2, ctx, _ = s.setup_sender(0, pkR, ikmE, info)
    ct2 = s.seal(ctx, pt, aad)
    good &= bool((ct2 == ct).all().item() and (enc2 == enc1).all().item())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731
    setup = [kem, kdf, 3, 0]

    def two_calls():
        nat.check(L.circl_hip_hpke_setup_sender_dev(*setup, p(pkR), p(ikmE), None, None, *info.args(), None, None, None, None, p(enc2), p(ctx), p(ok), n, st()), "setup")
        nat.check(L.circl_hip_hpke_seal_dev(3, p(ctx), s.CS, None, *pt.args(), *aad.args(), p(ct2), n, st()), "seal")

    calls = {
        "encap": lambda: nat.check(L.circl_hip_hpke_dhkem_encap_dev(kem, p(pkR), p(ikmE), p(enc), p(ss), p(ok), n, st()), "encap"),
        "seal_single": lambda: nat.check(L.circl_hip_hpke_seal_single_dev(*setup, p(pkR), p(ikmE), None, None, *info.args(), None, None, None, None, *pt.args(),
                                                                          *aad.args(), p(enc1), p(ct), p(ok1), n, st()), "seal_single"),
        "setup+seal": two_calls,
        "decap": lambda: nat.check(L.circl_hip_hpke_dhkem_decap_dev(kem, p(skR), p(pkR), p(enc), p(ss2), p(ok), n, st()), "decap"),
        "open_single": lambda: nat.check(L.circl_hip_hpke_open_single_dev(*setup, p(skR), p(pkR), p(enc1), None, *info.args(), None, None, None, None, p(ct),
                                                                          pt.off.data_ptr(), *aad.args(), p(back), p(ok2), n, st()), "open_single"),
    }
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, fn in calls.items():
            ms[name].append(_timed_for(fn, min_ms))
    mean = {name: sum(v) / len(v) for name, v in ms.items()}
    spread = {name: max(v) / min(v) - 1.0 for name, v in ms.items()}
    return dict(n=n, pt=pt_len, mean=mean, spread=spread, good=good)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,18")
    ap.add_argument("--pt", default="32,256,1024")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpke_seal_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/hpke_seal_bench.py needs a GPU: nothing is measured without one")
    L = nat.lib()
    rng = np.random.default_rng(9180)
    names = ["encap", "seal_single", "setup+seal", "decap", "open_single"]
    lines = ["python tools/hpke_seal_bench.py " + " ".join(sys.argv[1:]),
             "%s; ms per call (mean of %d passes) and spread = max / min - 1 of the passes; base mode, ChaCha20Poly1305, aad 8, info 20" %
             (torch.cuda.get_device_name(0), a.passes),
             "%-15s %8s %5s " % ("suite", "n", "pt") + " ".join("%12s %6s" % (x, "spread") for x in names) + "  seal/encap open/decap 2call/single  checked"]
    for kem, kdf, label in SUITES:
        for lg in [int(x) for x in a.sizes.split(",") if x]:
            for pt_len in [int(x) for x in a.pt.split(",") if x]:
                r = bench(L, kem, kdf, lg, pt_len, a.passes, a.min_ms, rng)
                m, sp = r["mean"], r["spread"]
                lines.append("%-15s %8d %5d " % (label, r["n"], r["pt"]) + " ".join("%12.4f %5.1f%%" % (m[x], 100 * sp[x]) for x in names) +
                             "  %10.3f %10.3f %12.3f  %s" % (m["seal_single"] / m["encap"], m["open_single"] / m["decap"], m["setup+seal"] / m["seal_single"],
                                                              "ok" if r["good"] else "MISMATCH"))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
