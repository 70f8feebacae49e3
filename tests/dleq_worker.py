"""Child process of the DLEQ host-pipeline tests (tests/test_gpu_dleq.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_ZEROCOPY_KB, CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/dleq_worker.py DEVICE N_REQ OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CTX = b"dleq_worker-ristretto255"
ORDER = 2**252 + 27742317777372353535851937790883648493
GUARD, FILL = 64, 0xA5


def scalars(rng, n):
    b = b"".join((1 + int.from_bytes(rng.bytes(32), "little") % (ORDER - 1)).to_bytes(32, "little") for _ in range(n))
    return np.frombuffer(b, np.uint8).reshape(n, 32).copy()


def inputs(api, n_req, device=0):
    """n_req requests of i % 4 + 1 elements under a key per request: (k, kA, B, kB, off, r).  B_j are small multiples of the generator
    (few distinct elements per request keep the checker cheap); kB = k B and kA = k G come from the scalar multiplication entry point."""
    rng = np.random.default_rng(2292)
    sizes = np.array([i % 4 + 1 for i in range(n_req)], np.int64)
    off = np.zeros(n_req + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    n_el = int(off[-1])
    k, r = scalars(rng, n_req), scalars(rng, n_req)
    small = np.zeros((n_el, 32), np.uint8)
    small[:, 0] = 1 + np.arange(n_el) % 5
    B, ok_b = api.ristretto255_scalar_mult(small, device=device)
    kB, ok_kb = api.ristretto255_scalar_mult(np.repeat(k, sizes, axis=0), B, device=device)
    kA, ok_ka = api.ristretto255_scalar_mult(k, device=device)
    assert ok_b.all() and ok_kb.all() and ok_ka.all()
    return k, kA, B, kB, off, r


def guarded(nbytes):
    a = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
    return a, C.c_void_p(a.ctypes.data + GUARD)


def unguard(a, nbytes, what):
    assert (a[:GUARD] == FILL).all() and (a[GUARD + nbytes:] == FILL).all(), what
    return a[GUARD:GUARD + nbytes].copy()


def run(api, device, n_req):
    """prove and verify through the host forms, outputs between guard margins; the inputs are made on device 0 by single-chunk calls.
    Then the POPRF item calls (run_items)."""
    from circl_amd import _native as nat
    lib = nat.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    k, kA, B, kB, off, r = inputs(api, n_req)
    ctx = np.frombuffer(CTX + b"\0", np.uint8)
    proofs, pp = guarded(64 * n_req)
    ok, po = guarded(n_req)
    nat.check(lib.circl_hip_dleq_prove(p(k), 32, p(kA), 32, p(B), p(kB), p(off), p(r), p(ctx), len(CTX), 1, pp, po, n_req, device), "dleq_prove")
    o = {"proofs": unguard(proofs, 64 * n_req, "proofs").reshape(n_req, 64), "ok": unguard(ok, n_req, "ok")}
    verdict, pv = guarded(n_req)
    nat.check(lib.circl_hip_dleq_verify(p(kA), 32, p(B), p(kB), p(off), p(o["proofs"]), p(ctx), len(CTX), 1, pv, n_req, device), "dleq_verify")
    o["verdict"] = unguard(verdict, n_req, "verdict")
    bad = o["proofs"].copy()
    bad[1::2, 40] ^= 4          # every second proof's s
    nat.check(lib.circl_hip_dleq_verify(p(kA), 32, p(B), p(kB), p(off), p(bad), p(ctx), len(CTX), 1, pv, n_req, device), "dleq_verify")
    o["verdict_bad"] = unguard(verdict, n_req, "verdict")
    o.update(run_items(api, device, n_req, k, kA, r))
    return o


def item_inputs(n):
    """(infos, inputs) of n POPRF items: infos of i % 7 bytes, inputs of i % 41 bytes (empty ones at both sides of the chunk boundary 255 | 256)"""
    rng = np.random.default_rng(9497)
    return [rng.bytes(i % 7) for i in range(n)], [rng.bytes(0 if i in (255, 256) else i % 41) for i in range(n)]


def run_items(api, device, n, k, kA, r):
    """the POPRF item calls through the host forms: the tweak with a key per item, with one key and on the client's side (one public key);
    Finalize and FullEvaluate with and without an info blob.  k are the keys (k[0] the shared one, kA[0] its public key), r the blinds, and
    kA stands in for the evaluated elements (Finalize takes any valid element)."""
    infos, ins = item_inputs(n)
    o = {}
    o["t"], o["tinv"], o["tw"], o["ok_tw"] = api.oprf_poprf_tweak(infos, sk=k, device=device)
    o["t1"], o["tinv1"], o["tw1"], o["ok_tw1"] = api.oprf_poprf_tweak(infos, sk=k[0].tobytes(), device=device)
    o["twc"], o["ok_twc"] = api.oprf_poprf_tweak(infos, pkS=kA[0].tobytes(), device=device)
    o["pfin"], o["ok_pfin"] = api.oprf_poprf_finalize(ins, infos, r, kA, device=device)
    o["pfin0"], o["ok_pfin0"] = api.oprf_poprf_finalize(ins, None, r, kA, device=device)
    o["pfull"], o["ok_pfull"] = api.oprf_poprf_full_evaluate(k, ins, infos, device=device)
    o["pfull0"], o["ok_pfull0"] = api.oprf_poprf_full_evaluate(k[0].tobytes(), ins, None, device=device)
    return o


def main(device, n, dst):
    from circl_amd import hostapi as api
    np.savez(dst, **run(api, int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
