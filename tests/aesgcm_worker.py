"""Child process of the AES-GCM host-pipeline tests (tests/test_gpu_aesgcm.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_ZEROCOPY_KB, CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/aesgcm_worker.py DEVICE N OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# "rows": AES-128, context-row layout -- a key per item at +0 and a nonce per item at +32 of rows of ROW bytes, explicit nonces;
# "run": AES-256, one key and one base nonce for the batch (both strides 0), seq = SEQ0 + i
KEYINGS = (("rows", 16), ("run", 32))
ROW = 80
SEQ0 = 250                                                  # the run crosses sequence number 255 | 256
FORGED = (255, 256, 299)
FORGED_TAG = 100                                            # the first item of the second shard, in the Open over rows of tags
GUARD, FILL = 64, 0xA5


def inputs(n):
    """n items: rows of ROW bytes of noise (key at +0, nonce at +32), the one AES-256 key and base nonce, plaintexts of i % 37 bytes
    (empty ones at both sides of the chunk boundary 255 | 256), aads of i % 11 bytes"""
    rng = np.random.default_rng(38)
    rows = rng.integers(0, 256, (n, ROW), dtype=np.uint8)
    key, base = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 12, dtype=np.uint8)
    pts = [rng.bytes(0 if i in (255, 256) else i % 37) for i in range(n)]
    aads = [rng.bytes(i % 11) for i in range(n)]
    return rows, key, base, pts, aads


def keying(name, i, n):
    """(key, nonce) of item i as the checker wants them"""
    import aesgcm
    rows, key, base, _, _ = inputs(n)
    if name == "rows":
        return rows[i, :16].tobytes(), rows[i, 32:44].tobytes()
    return key.tobytes(), aesgcm.seq_nonce(base.tobytes(), SEQ0 + i)


def blob(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items) + b"\0", np.uint8).copy(), off


def run(L, device, n):
    """per keying: Seal (with and without an aad blob), Open of what it made, Open with the tags of FORGED flipped, Seal without a plaintext
    blob (rows of 16 tags) and Open over those rows with FORGED_TAG's flipped.  Every output lies between guard margins; `guards` = every
    margin still holds its fill value."""
    from circl_amd import _native as nat
    p = lambda a, at=0: None if a is None else C.c_void_p(a.ctypes.data + at)
    rows, key, base, pts, aads = inputs(n)
    seq = np.arange(SEQ0, SEQ0 + n, dtype=np.uint64)
    (pb, off), (ab, ao) = blob(pts), blob(aads)
    P, CT = int(off[n]), int(off[n]) + 16 * n
    held, o = [], {}

    def guarded(nbytes):
        buf = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
        held.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    for name, kb in KEYINGS:
        head = (kb, p(rows), ROW, p(rows, 32), ROW, None) if name == "rows" else (kb, p(key), 0, p(base), 0, p(seq))
        seal = lambda pt, po, a, aoff, ct: nat.check(L.circl_hip_aesgcm_seal(*head, p(pt), p(po), p(a), p(aoff), p(ct), n, device), "aesgcm_seal")
        opn = lambda ct, po, pt, ok: nat.check(L.circl_hip_aesgcm_open(*head, p(ct), p(po), p(ab), p(ao), p(pt), p(ok), n, device), "aesgcm_open")
        ct, ct_noaad, pt, fpt, tags, none = guarded(CT), guarded(CT), guarded(P), guarded(P), guarded(16 * n), guarded(0)
        ok, fok, tok = guarded(n), guarded(n), guarded(n)
        seal(pb, off, ab, ao, ct)
        seal(pb, off, None, None, ct_noaad)
        opn(ct, off, pt, ok)
        forged = ct.copy()
        for i in FORGED:
            forged[int(off[i + 1]) + 16 * (i + 1) - 1] ^= 0x10
        opn(forged, off, fpt, fok)
        seal(None, None, ab, ao, tags)
        bad_tags = tags.copy()
        bad_tags[16 * FORGED_TAG + 15] ^= 1
        opn(bad_tags, None, none, tok)
        for k, a in (("ct", ct), ("ct_noaad", ct_noaad), ("pt", pt), ("fpt", fpt), ("tags", tags), ("ok", ok), ("fok", fok), ("tok", tok)):
            o[name + "_" + k] = a.copy()
    o["guards"] = np.array([(b[:GUARD] == FILL).all() and (b[GUARD + nb:] == FILL).all() for b, nb in held])
    return o


def main(device, n, dst):
    from circl_amd import _native as nat
    np.savez(dst, **run(nat.lib(), int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
