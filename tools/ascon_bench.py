#!/usr/bin/env python3
"""Batch Ascon128 / Ascon128a / Ascon80pq Seal and Open rates on one GPU (the _dev forms).

    python tools/ascon_bench.py [--sizes 10,14,18] [--lens 64,1350,8192] [--aad 13] [--passes 3] [--min-ms 200] [--alt LIB]
                                [--out profiles/ascon_bench.txt]

Per mode, plaintext length and batch size n (the reference's BenchmarkAscon shapes: 64, 1350 and 8192 bytes with 13 bytes of aad; n = 2^18
becomes 2^16 at 8192 bytes so that the buffers stay near 0.5 GB): circl_hip_ascon_seal_dev and circl_hip_ascon_open_dev on resident
tensors, a key and a nonce per item, uniform lengths (item i's plaintext starts at i * length, so at 1350 bytes every other item is
4-byte aligned and at 64 / 8192 bytes all are).  Device events around at least --min-ms of back-to-back calls after a warm-up, alternated
over --passes passes.  Each figure: plaintext bytes per second and items per second from the mean of the passes, and the spread
(max / min - 1) of the passes.  Open(Seal(pt)) == pt with ok all 1 is checked at every shape.

--alt LIB times a second build of the library (another variant of the kernels) in the same process, alternated call by call with the
tree's own, and adds its rates and the ratio own / alt: how the byte-wise and the word-wise memory path were compared.  Its ciphertexts
must equal the tree's own.

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

MODES = (("Ascon128", 1), ("Ascon128a", 2), ("Ascon80pq", -1))
STATIC = ("static figures (hipcc --offload-arch=gfx950 -O3, -save-temps disassembly and -Rpass-analysis=kernel-resource-usage; not measurements): "
          "52 VALU per round (21 v_bitop3_b32, 20 v_alignbit_b32, 11 v_xor_b32) = 39 per byte for Ascon128 / Ascon80pq (6 rounds per 8 bytes), 26 for "
          "Ascon128a (8 per 16); __launch_bounds__(64, 8) asks for at most 64 VGPRs; Seal / Open kernels: Ascon128 44 / 50 VGPRs, Ascon128a 43 / 47, "
          "Ascon80pq 45 / 51; scratch 0 bytes per lane, no LDS, occupancy 8 waves per SIMD in all six")


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


def load_alt(path):
    L = C.CDLL(os.path.abspath(path))
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.circl_hip_ascon_seal_dev.argtypes = [i, vp, sz, vp] + [vp] * 5 + [sz, vp]
    L.circl_hip_ascon_open_dev.argtypes = [i, vp, sz, vp] + [vp] * 6 + [sz, vp]
    return L


def bench(libs, mode, length, aad_len, n, passes, min_ms, rng):
    """-> {lib name: {"seal": [ms per pass], "open": [...]}}, everything checked"""
    ks = nat.lib().circl_hip_ascon_key_size(mode)
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    keys, nonces = t(rng.integers(0, 256, (n, ks), dtype=np.uint8)), t(rng.integers(0, 256, (n, 16), dtype=np.uint8))
    pt = torch.randint(0, 256, (n * length + 16,), dtype=torch.uint8, device="cuda")
    aad = torch.randint(0, 256, (n * aad_len + 16,), dtype=torch.uint8, device="cuda")
    off, aoff = t(np.arange(n + 1, dtype=np.int64) * length), t(np.arange(n + 1, dtype=np.int64) * aad_len)
    ct = {k: torch.empty(n * (length + 16), dtype=torch.uint8, device="cuda") for k in libs}
    back, ok = torch.empty(n * length + 16, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def seal(k):
        nat.check(libs[k].circl_hip_ascon_seal_dev(mode, keys.data_ptr(), ks, nonces.data_ptr(), pt.data_ptr(), off.data_ptr(), aad.data_ptr(), aoff.data_ptr(),
                                                   ct[k].data_ptr(), n, st()), "ascon_seal_dev")

    def open_(k):
        nat.check(libs[k].circl_hip_ascon_open_dev(mode, keys.data_ptr(), ks, nonces.data_ptr(), ct[k].data_ptr(), off.data_ptr(), aad.data_ptr(), aoff.data_ptr(),
                                                   back.data_ptr(), ok.data_ptr(), n, st()), "ascon_open_dev")

    good = True
    for k in libs:
        seal(k)
        back.zero_()
        open_(k)
        torch.cuda.synchronize()
        good &= bool(ok.all().item() and (back[:n * length] == pt[:n * length]).all().item() and (ct[k] == ct["own"]).all().item())
    ms = {k: {"seal": [], "open": []} for k in libs}
    for _ in range(passes):
        for op, fn in (("seal", seal), ("open", open_)):
            for k in libs:
                ms[k][op].append(_timed_for(lambda: fn(k), min_ms))
    return ms, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,18")
    ap.add_argument("--lens", default="64,1350,8192")
    ap.add_argument("--aad", type=int, default=13)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--alt", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ascon_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ascon_bench.py needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(128)
    libs = {"own": nat.lib()}
    if a.alt:
        libs["alt"] = load_alt(a.alt)
    head = "%-10s %6s %8s" % ("mode", "bytes", "n")
    for k in libs:
        for op in ("seal", "open"):
            head += " %11s %11s %6s" % (("%s %s B/s" % (k, op)), "items/s", "spread")
    if a.alt:
        head += "  own/alt seal   open"
    lines = ["python tools/ascon_bench.py " + " ".join(sys.argv[1:]),
             "%s; _dev forms, %d bytes of aad, a key and a nonce per item; plaintext bytes per second and items per second from the mean ms per call of %d passes, "
             "spread = max / min - 1 of the passes%s" % (torch.cuda.get_device_name(0), a.aad, a.passes, "; alt = " + a.alt if a.alt else ""),
             STATIC, head]
    worst = 0.0
    for name, mode in MODES:
        for length in [int(x) for x in a.lens.split(",") if x]:
            for lg in [int(x) for x in a.sizes.split(",") if x]:
                n = 1 << (min(lg, 16) if length >= 8192 else lg)
                ms, good = bench(libs, mode, length, a.aad, n, a.passes, a.min_ms, rng)
                row = "%-10s %6d %8d" % (name, length, n)
                mean = {}
                for k in libs:
                    for op in ("seal", "open"):
                        v = ms[k][op]
                        mean[k, op] = sum(v) / len(v)
                        spread = max(v) / min(v) - 1.0
                        worst = max(worst, spread)
                        row += " %11.4g %11.4g %5.1f%%" % (n * length / mean[k, op] * 1e3, n / mean[k, op] * 1e3, 100 * spread)
                if a.alt:
                    row += "  %12.3f %6.3f" % (mean["alt", "seal"] / mean["own", "seal"], mean["alt", "open"] / mean["own", "open"])
                row += "  ok" if good else "  MISMATCH"
                lines.append(row)
                print(row, flush=True)
                torch.cuda.empty_cache()
    lines.append("largest spread of any figure above: %.1f%%" % (100 * worst))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4] + lines[-1:]))


if __name__ == "__main__":
    main()
