"""Child process of the NIST-curve DLEQ host-pipeline tests (tests/test_gpu_dleq_nistp.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/dleq_nistp_worker.py CURVE DEVICE N_REQ OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX = b"dleq_nistp_worker"
ORDER = {256: 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551,
         384: 0xffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973}
GUARD, FILL = 64, 0xA5


def scalars(rng, curve, n):
    ns = curve // 8
    b = b"".join((1 + int.from_bytes(rng.bytes(ns), "big") % (ORDER[curve] - 1)).to_bytes(ns, "big") for _ in range(n))
    return np.frombuffer(b, np.uint8).reshape(n, ns).copy()


def inputs(api, curve, n_req):
    """n_req requests of i % 4 + 1 elements under a key per request: (k, kA, B, kB, off, r, b).  B_j = b_j G for b_j in 1 .. 5 (the
    checker then needs one multiplication per request); kB = k B and kA = k G come from the scalar multiplication entry point, on device
    0 in single-chunk calls."""
    o = api.NistpOprf(curve)
    rng = np.random.default_rng(2292 + curve)
    sizes = np.array([i % 4 + 1 for i in range(n_req)], np.int64)
    off = np.zeros(n_req + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    n_el = int(off[-1])
    k, r = scalars(rng, curve, n_req), scalars(rng, curve, n_req)
    small = np.zeros((n_el, o.Ns), np.uint8)
    b = 1 + np.arange(n_el) % 5
    small[:, -1] = b
    B, ok_b = o.scalar_mult(small)
    kB, ok_kb = o.scalar_mult(np.repeat(k, sizes, axis=0), B)
    kA, ok_ka = o.scalar_mult(k)
    assert ok_b.all() and ok_kb.all() and ok_ka.all()
    return k, kA, B, kB, off, r, b


def guarded(nbytes):
    a = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
    return a, C.c_void_p(a.ctypes.data + GUARD)


def unguard(a, nbytes, what):
    assert (a[:GUARD] == FILL).all() and (a[GUARD + nbytes:] == FILL).all(), what
    return a[GUARD:GUARD + nbytes].copy()


def item_inputs(n):
    """(infos, inputs) of n POPRF items: infos of i % 7 bytes, inputs of i % 41 bytes (empty ones at both sides of the chunk boundary 255 | 256)"""
    rng = np.random.default_rng(9497)
    return [rng.bytes(i % 7) for i in range(n)], [rng.bytes(0 if i in (255, 256) else i % 41) for i in range(n)]


def run(api, curve, device, n_req):
    """prove and verify through the host forms, outputs between guard margins; then the POPRF item calls through the wrappers: the tweak
    with a key per item, with one key and on the client's side; Finalize and FullEvaluate with and without an info blob (kA stands in
    for the evaluated elements: Finalize takes any valid element)."""
    from circl_amd import _native as nat
    lib = nat.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ns, ne = curve // 8, curve // 8 + 1
    k, kA, B, kB, off, r, _ = inputs(api, curve, n_req)
    ctx = np.frombuffer(CTX + b"\0", np.uint8)
    proofs, pp = guarded(2 * ns * n_req)
    ok, po = guarded(n_req)
    nat.check(lib.circl_hip_nistp_dleq_prove(curve, p(k), ns, p(kA), ne, p(B), p(kB), p(off), p(r), p(ctx), len(CTX), 1, pp, po, n_req, device), "nistp_dleq_prove")
    o = {"proofs": unguard(proofs, 2 * ns * n_req, "proofs").reshape(n_req, 2 * ns), "ok": unguard(ok, n_req, "ok")}
    verdict, pv = guarded(n_req)
    nat.check(lib.circl_hip_nistp_dleq_verify(curve, p(kA), ne, p(B), p(kB), p(off), p(o["proofs"]), p(ctx), len(CTX), 1, pv, n_req, device), "nistp_dleq_verify")
    o["verdict"] = unguard(verdict, n_req, "verdict")
    bad = o["proofs"].copy()
    bad[1::2, ns + 8] ^= 4          # every second proof's s
    nat.check(lib.circl_hip_nistp_dleq_verify(curve, p(kA), ne, p(B), p(kB), p(off), p(bad), p(ctx), len(CTX), 1, pv, n_req, device), "nistp_dleq_verify")
    o["verdict_bad"] = unguard(verdict, n_req, "verdict")
    w = api.NistpOprf(curve, device)
    infos, ins = item_inputs(n_req)
    o["t"], o["tinv"], o["tw"], o["ok_tw"] = w.poprf_tweak(infos, sk=k)
    o["t1"], o["tinv1"], o["tw1"], o["ok_tw1"] = w.poprf_tweak(infos, sk=k[0].tobytes())
    o["twc"], o["ok_twc"] = w.poprf_tweak(infos, pkS=kA[0].tobytes())
    o["pfin"], o["ok_pfin"] = w.poprf_finalize(ins, infos, r, kA)
    o["pfin0"], o["ok_pfin0"] = w.poprf_finalize(ins, None, r, kA)
    o["pfull"], o["ok_pfull"] = w.poprf_full_evaluate(k, ins, infos)
    o["pfull0"], o["ok_pfull0"] = w.poprf_full_evaluate(k[0].tobytes(), ins, None)
    return o


def main(curve, device, n, dst):
    from circl_amd import hostapi as api
    np.savez(dst, **run(api, int(curve), int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:5])
