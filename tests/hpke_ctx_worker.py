"""Child process of the HPKE host-pipeline tests (tests/test_gpu_hpke_ctx.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_ZEROCOPY_KB, CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/hpke_ctx_worker.py DEVICE IN.npz OUT.npz

IN holds pkR, skR, ikmE (n, 32); OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SUITE = (0x20, 1, 3)
FORGED = (255, 256, 299)
FORGED_TAG = 100   # in the Open over rows of tags: the first item of the second shard
EXPORT_L = 33
GUARD, FILL = 64, 0xA5


def inputs(n):
    """(plaintexts, aads, sequence numbers) of n items: plaintexts of i % 37 bytes (empty ones at 0, 37, .. and at both sides of the
    chunk boundary 255 | 256), aads of i % 9 bytes, sequence numbers 3 i"""
    rng = np.random.default_rng(37)
    pts = [rng.integers(0, 256, 0 if i in (255, 256) else i % 37, dtype=np.uint8).tobytes() for i in range(n)]
    aads = [rng.integers(0, 256, i % 9, dtype=np.uint8).tobytes() for i in range(n)]
    return pts, aads, [3 * i for i in range(n)]


def flip_tag(ct):
    return ct[:-1] + bytes([ct[-1] ^ 0x10])


def _flat(items):
    return np.frombuffer(b"".join(items), np.uint8)


def run(api, pkR, skR, ikmE, device):
    """every host form that reads or writes a ragged blob, through HpkeSuite; then the same four entry points once more through ctypes
    into blobs with a guard margin on both sides (`guards` = every margin still holds its fill value, `guarded_same` = the blobs
    between the margins equal HpkeSuite's), Seal without a plaintext blob and Open over those rows of tags; then Export and its single-shot
    forms, and every setup and single-shot form once more in mode 3 (run_auth_psk)"""
    from circl_amd import _native as nat
    h = api.HpkeSuite(*SUITE, device=device)
    n = len(pkR)
    pts, aads, seq = inputs(n)
    o = {}
    o["enc"], ctx, o["ok_s"] = h.setup_sender(0, pkR, ikmE)
    ctx_r, o["ok_r"] = h.setup_receiver(0, skR, o["enc"])
    o["ctx"], o["ctx_r"] = ctx, ctx_r
    cts = h.seal(ctx, pts, aads, seq)
    back, o["ok"] = h.open(ctx_r, cts, aads, seq)
    forged = [flip_tag(c) if i in FORGED else c for i, c in enumerate(cts)]
    fpt, o["fok"] = h.open(ctx_r, forged, aads, seq)
    o["enc1"], ct1, o["ok1"] = h.seal_single(0, pkR, ikmE, pts, aads)
    pt1, o["ok1r"] = h.open_single(0, skR, o["enc1"], ct1, aads)
    o.update(ct=_flat(cts), pt=_flat(back), fpt=_flat(fpt), ct1=_flat(ct1), pt1=_flat(pt1), ct_noaad=_flat(h.seal(ctx, pts, None, seq)))

    L, p, po = h.L, api._p, api._po
    (pb, off), (ab, ao), sq = api._blob(pts), api._blob(aads), np.array(seq, np.uint64)
    P, CT = int(off[n]), int(off[n]) + 16 * n
    held = []

    def guarded(nbytes):
        buf = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
        held.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    _, sargs, keep_s = h._setup_args(0, (pkR, ikmE, None, None), None, None, None)
    _, rargs, keep_r = h._setup_args(0, (skR, None, o["enc"], None), None, None, None)
    g_ct, g_pt, g_ct1, g_pt1, g_tags = guarded(CT), guarded(P), guarded(CT), guarded(P), guarded(16 * n)
    ok, enc = np.empty(n, np.uint8), np.empty((n, 32), np.uint8)
    nat.check(L.circl_hip_hpke_seal(3, p(ctx), h.CS, p(sq), p(pb), p(off), p(ab), p(ao), p(g_ct), n, device), "seal")
    nat.check(L.circl_hip_hpke_open(3, p(ctx_r), h.CS, p(sq), p(g_ct), p(off), p(ab), p(ao), p(g_pt), p(ok), n, device), "open")
    nat.check(L.circl_hip_hpke_seal_single(*sargs, p(pb), p(off), p(ab), p(ao), p(enc), p(g_ct1), p(ok), n, device), "seal_single")
    nat.check(L.circl_hip_hpke_open_single(*rargs, p(g_ct1), p(off), p(ab), p(ao), p(g_pt1), p(ok), n, device), "open_single")
    # Seal without a plaintext blob: every plaintext is empty, the ciphertexts are n tags
    nat.check(L.circl_hip_hpke_seal(3, p(ctx), h.CS, p(sq), None, None, p(ab), p(ao), p(g_tags), n, device), "seal without plaintexts")
    o["tags"] = g_tags.copy()
    o["guarded_same"] = np.array([(g_ct == o["ct"]).all(), (g_pt == o["pt"]).all(), (g_ct1 == o["ct1"]).all(), (g_pt1 == o["pt1"]).all()])
    # Open without offsets: the ciphertexts are rows of tags, FORGED_TAG's is forged; no plaintext byte is written
    bad_tags, g_none, o["tok"] = g_tags.copy(), guarded(0), np.empty(n, np.uint8)
    bad_tags[16 * FORGED_TAG + 15] ^= 1
    nat.check(L.circl_hip_hpke_open(3, p(ctx_r), h.CS, p(sq), p(bad_tags), None, p(ab), p(ao), p(g_none), p(o["tok"]), n, device), "open of rows of tags")
    o["guards"] = np.array([(b[:GUARD] == FILL).all() and (b[GUARD + nb:] == FILL).all() for b, nb in held])
    # Export on context rows and its two single-shot forms
    exps = exporter_contexts(n)
    o["exp"] = h.export(ctx, exps, EXPORT_L)
    o["enc_x"], o["exp1"], o["ok_x"] = h.export_single(0, pkR, ikmE, exps, EXPORT_L)
    o["exp1r"], o["ok_xr"] = h.export_single_receiver(0, skR, o["enc_x"], exps, EXPORT_L)
    o.update(run_auth_psk(api, h, pkR, skR, ikmE, device))
    return o


def exporter_contexts(n):
    rng = np.random.default_rng(33)
    return [rng.bytes(i % 13) for i in range(n)]


def auth_psk_inputs(n):
    """(the sender's ikm rows, infos of i % 8 bytes, psks of 32 + i % 5 bytes, psk ids of 1 + i % 6 bytes)"""
    rng = np.random.default_rng(3)
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), [rng.bytes(i % 8) for i in range(n)], [rng.bytes(32 + i % 5) for i in range(n)],
            [rng.bytes(1 + i % 6) for i in range(n)])


def run_auth_psk(api, h, pkR, skR, ikmE, device):
    """the second pass, in mode 3 (auth + PSK): the sender's key rows, the psk and psk id blobs and the info blob are staged too"""
    n = len(pkR)
    pts, aads, _ = inputs(n)
    ikmS, infos, psks, ids = auth_psk_inputs(n)
    skS, pkS = api.hpke_dhkem_derive_keypair(SUITE[0], ikmS, device=device)
    exps, o = exporter_contexts(n), {"skS": skS, "pkS": pkS}
    o["enc3"], o["ctx3"], o["ok3_s"] = h.setup_sender(3, pkR, ikmE, infos, psks, ids, skS=skS, pkS=pkS)
    o["ctx3_r"], o["ok3_r"] = h.setup_receiver(3, skR, o["enc3"], infos, psks, ids, pkS=pkS, pkR=pkR)
    o["enc3_1"], ct, o["ok3_1"] = h.seal_single(3, pkR, ikmE, pts, aads, infos, psks, ids, skS=skS, pkS=pkS)
    pt, o["ok3_1r"] = h.open_single(3, skR, o["enc3_1"], ct, aads, infos, psks, ids, pkS=pkS, pkR=pkR)
    o["ct3_1"], o["pt3_1"] = _flat(ct), _flat(pt)
    o["enc3_x"], o["exp3"], o["ok3_x"] = h.export_single(3, pkR, ikmE, exps, EXPORT_L, infos, psks, ids, skS=skS, pkS=pkS)
    o["exp3_r"], o["ok3_xr"] = h.export_single_receiver(3, skR, o["enc3_x"], exps, EXPORT_L, infos, psks, ids, pkS=pkS, pkR=pkR)
    return o


def main(device, src, dst):
    from circl_amd import hostapi as api
    d = np.load(src)
    np.savez(dst, **run(api, d["pkR"], d["skR"], d["ikmE"], int(device)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
