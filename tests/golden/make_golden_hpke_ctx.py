#!/usr/bin/env python3
"""Writes tests/golden/hpke_ctx.json.gz from the reference checkout (data only: the RFC 9180 vectors that hpke/vectors_test.go
reads, with their key-schedule, encryption and export fields).  Run in the build container only (the GPU box has no reference
checkout):
    python tests/golden/make_golden_hpke_ctx.py

From hpke/testdata/vectors_rfc9180_5f503c5.json.gz the 32 vectors with kem_id 32 / 33 (X25519 / X448), kdf_id 1 / 3 (HKDF-SHA256 /
HKDF-SHA512) and aead_id 3 / 65535 (ChaCha20Poly1305 / export-only): one per mode for each triple.  Kept per vector: what
make_golden_hpke.py keeps, plus kdf_id, aead_id, info, psk, psk_id, key_schedule_context, secret, key, base_nonce,
exporter_secret, all 3 exports, and of the 257 encryptions those at sequence numbers 0, 1, 2, 4, 255 and 256 (each with its "seq";
256 is the first whose nonce differs from the base nonce in the second counter byte).  All binary fields are hex strings.
"""
import gzip
import json
import os

from make_golden_hpke import FIELDS, REF

OUT = os.path.dirname(os.path.abspath(__file__))
MORE = ("kdf_id", "aead_id", "info", "psk", "psk_id", "key_schedule_context", "secret", "key", "base_nonce", "exporter_secret", "exports")
SEQS = (0, 1, 2, 4, 255, 256)


def main():
    with gzip.open(os.path.join(REF, "hpke/testdata/vectors_rfc9180_5f503c5.json.gz"), "rt") as f:
        vectors = json.load(f)
    data = []
    for v in vectors:
        if v["kem_id"] not in (32, 33) or v["kdf_id"] not in (1, 3) or v["aead_id"] not in (3, 65535):
            continue
        d = {k: v[k] for k in FIELDS + MORE if k in v}
        d["encryptions"] = [dict(v["encryptions"][s], seq=s) for s in SEQS] if v["encryptions"] else []
        data.append(d)
    with gzip.GzipFile(os.path.join(OUT, "hpke_ctx.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("hpke_ctx.json.gz: %d vectors, %d encryptions" % (len(data), sum(len(d["encryptions"]) for d in data)))


if __name__ == "__main__":
    main()
