#!/usr/bin/env python3
"""Batch AES-128-GCM / AES-256-GCM Seal and Open rates on one GPU (the _dev forms), beside Ascon128 and ChaCha20-Poly1305.

    python tools/aesgcm_bench.py [--shapes 18x64,18x1350,16x8192] [--aad 13] [--passes 3] [--min-ms 200] [--alt LIB]
                                 [--out profiles/aesgcm_bench.txt]

Per shape (2^lg items x plaintext bytes; the shapes of tools/ascon_bench.py) and key size: circl_hip_aesgcm_seal_dev and _open_dev on
resident tensors with a key and a nonce per item, and with one key for the batch (key_stride 0); uniform lengths (item i's plaintext
starts at i * length).  In the same process and the same passes, alternated call kind by call kind: circl_hip_ascon_seal_dev (Ascon128, a
key per item) and circl_hip_hpke_seal_dev (ChaCha20-Poly1305 on stored context rows of 80 bytes) at the same shape.  Device events around at
least --min-ms of back-to-back calls after a warm-up, over --passes passes.  Each figure: plaintext bytes per second from the mean of the
passes, and the spread (max / min - 1) of the passes; the two ratios are AES-GCM Seal (a key per item) over Ascon128 Seal and over
ChaCha20-Poly1305 Seal.  Open(Seal(pt)) == pt with ok all 1 is checked at every shape.

--alt LIB times a second build of the library (another variant of the AES-GCM kernels) in the same process, alternated with the tree's
own, and adds its rates and the ratio own / alt.  Its ciphertexts must equal the tree's own.

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

STATIC = ("static figures (hipcc --offload-arch=gfx950 -O3, -save-temps disassembly and kernel metadata; not measurements): Seal / Open kernels: AES-128 117 / 115 "
          "VGPRs, scratch 0 / 0 bytes per lane; AES-256 128 / 127 VGPRs, scratch 20 / 0 (4 spilled VGPRs in Seal); no LDS, occupancy 4 in all four.  One two-block "
          "AES pass (32 bytes): 2777 - 2815 VALU instructions for AES-128, 3833 - 3872 for AES-256 (per round ~277: the 113-gate S-box, ShiftRows, MixColumns, the "
          "widening AddRoundKey); the key schedule 1575 / 2028; one ghash_mul (16 bytes): 32 iterations of 30 VALU (16 v_bitop3_b32, 3 v_alignbit_b32, 4 + 4 for the "
          "masks, 3 for the carry) + about 67 around them, about 1030 in all.  That is 87 + 64 = 151 VALU per byte for AES-128-GCM and 121 + 64 = 185 for AES-256-GCM "
          "on long items.")


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
    L.circl_hip_aesgcm_seal_dev.argtypes = [i, vp, sz, vp, sz] + [vp] * 6 + [sz, vp]
    L.circl_hip_aesgcm_open_dev.argtypes = [i, vp, sz, vp, sz] + [vp] * 7 + [sz, vp]
    return L


def bench(libs, length, aad_len, n, passes, min_ms, rng):
    """-> ({call kind: [ms per pass]}, everything checked).  Call kinds: (lib, key bytes, 'item' | 'shared', 'seal' | 'open'), 'ascon', 'chapoly'."""
    L = nat.lib()
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rows = t(rng.integers(0, 256, (n, 80), dtype=np.uint8))          # key at +0, nonce at +32: AES keys, Ascon keys and HPKE context rows alike
    nonces = t(rng.integers(0, 256, (n, 16), dtype=np.uint8))        # rows of 16: AES-GCM reads 12 of them, Ascon all
    pt = torch.randint(0, 256, (n * length + 16,), dtype=torch.uint8, device="cuda")
    aad = torch.randint(0, 256, (n * aad_len + 16,), dtype=torch.uint8, device="cuda")
    off, aoff = t(np.arange(n + 1, dtype=np.int64) * length), t(np.arange(n + 1, dtype=np.int64) * aad_len)
    seq = t(np.arange(n, dtype=np.int64))
    ct = {k: torch.empty(n * (length + 16), dtype=torch.uint8, device="cuda") for k in libs}
    other = torch.empty(n * (length + 16), dtype=torch.uint8, device="cuda")
    back, ok = torch.empty(n * length + 16, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def seal(k, kb, stride):
        nat.check(libs[k].circl_hip_aesgcm_seal_dev(kb, rows.data_ptr(), stride, nonces.data_ptr(), 16, None, pt.data_ptr(), off.data_ptr(), aad.data_ptr(),
                                                    aoff.data_ptr(), ct[k].data_ptr(), n, st()), "aesgcm_seal_dev")

    def open_(k, kb, stride):
        nat.check(libs[k].circl_hip_aesgcm_open_dev(kb, rows.data_ptr(), stride, nonces.data_ptr(), 16, None, ct[k].data_ptr(), off.data_ptr(), aad.data_ptr(),
                                                    aoff.data_ptr(), back.data_ptr(), ok.data_ptr(), n, st()), "aesgcm_open_dev")

    def ascon():
        nat.check(L.circl_hip_ascon_seal_dev(1, rows.data_ptr(), 80, nonces.data_ptr(), pt.data_ptr(), off.data_ptr(), aad.data_ptr(), aoff.data_ptr(),
                                             other.data_ptr(), n, st()), "ascon_seal_dev")

    def chapoly():
        nat.check(L.circl_hip_hpke_seal_dev(3, rows.data_ptr(), 80, seq.data_ptr(), pt.data_ptr(), off.data_ptr(), aad.data_ptr(), aoff.data_ptr(),
                                            other.data_ptr(), n, st()), "hpke_seal_dev")

    good = True
    kinds = {"ascon": ascon, "chapoly": chapoly}
    for kb in (16, 32):
        for keying, stride in (("item", 80), ("shared", 0)):
            for k in libs:
                seal(k, kb, stride)
                back.zero_()
                open_(k, kb, stride)
                torch.cuda.synchronize()
                good &= bool(ok.all().item() and (back[:n * length] == pt[:n * length]).all().item() and (ct[k] == ct["own"]).all().item())
                kinds[k, kb, keying, "seal"] = lambda k=k, kb=kb, stride=stride: seal(k, kb, stride)
                kinds[k, kb, keying, "open"] = lambda k=k, kb=kb, stride=stride: open_(k, kb, stride)
    ms = {kind: [] for kind in kinds}
    for _ in range(passes):
        for kind, fn in kinds.items():
            ms[kind].append(_timed_for(fn, min_ms))
    return ms, good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="18x64,18x1350,16x8192")
    ap.add_argument("--aad", type=int, default=13)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--alt", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aesgcm_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/aesgcm_bench.py needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(38)
    libs = {"own": nat.lib()}
    if a.alt:
        libs["alt"] = load_alt(a.alt)
    lines = ["python tools/aesgcm_bench.py " + " ".join(sys.argv[1:]),
             "%s; _dev forms, %d bytes of aad; plaintext bytes per second from the mean ms per call of %d passes, spread = max / min - 1 of the passes%s"
             % (torch.cuda.get_device_name(0), a.aad, a.passes, "; alt = " + a.alt if a.alt else ""), STATIC,
             "%-22s %6s %8s %11s %6s %11s %6s %9s %9s%s" % ("call", "bytes", "n", "seal B/s", "spread", "open B/s", "spread", "/ascon", "/chapoly",
                                                         "   own/alt seal   open" if a.alt else "")]
    worst = 0.0
    for shape in a.shapes.split(","):
        lg, length = (int(x) for x in shape.split("x"))
        n = 1 << lg
        ms, good = bench(libs, length, a.aad, n, a.passes, a.min_ms, rng)
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        spread = {k: max(v) / min(v) - 1.0 for k, v in ms.items()}
        worst = max(worst, max(spread.values()))
        rate = lambda kind: n * length / mean[kind] * 1e3  # noqa: E731
        for kind, label in (("ascon", "Ascon128 seal"), ("chapoly", "ChaCha20-Poly1305 seal")):
            lines.append("%-22s %6d %8d %11.4g %5.1f%%" % (label, length, n, rate(kind), 100 * spread[kind]))
        for k in libs:
            for kb in (16, 32):
                for keying in ("item", "shared"):
                    s, o = (k, kb, keying, "seal"), (k, kb, keying, "open")
                    row = "%-22s %6d %8d %11.4g %5.1f%% %11.4g %5.1f%% %9.3f %9.3f" % (
                        "%sAES-%d-GCM %s key" % ("alt " if k == "alt" else "", 8 * kb, keying), length, n, rate(s), 100 * spread[s], rate(o), 100 * spread[o],
                        mean["ascon"] / mean[s], mean["chapoly"] / mean[s])
                    if a.alt and k == "alt":
                        row += "   %12.3f %6.3f" % (mean[s] / mean["own", kb, keying, "seal"], mean[o] / mean["own", kb, keying, "open"])
                    lines.append(row + ("  ok" if good else "  MISMATCH"))
        print("\n".join(lines[-(2 + 4 * len(libs)):]), flush=True)
        torch.cuda.empty_cache()
    lines.append("largest spread of any figure above: %.1f%%" % (100 * worst))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4] + lines[-1:]))


if __name__ == "__main__":
    main()
