#!/usr/bin/env python3
"""Writes tests/golden/aesgcm_hpke.json.gz from the reference checkout (data only: the AES-GCM known answers inside the RFC 9180
vectors that hpke/vectors_test.go reads).  Run in the build container only (the GPU box has no reference checkout):
    python tests/golden/make_golden_aesgcm.py

From hpke/testdata/vectors_rfc9180_5f503c5.json.gz the 64 vectors with aead_id 1 / 2 (AES-128-GCM / AES-256-GCM): 4 KEMs x 2 KDFs x
2 AEADs x 4 modes.  Whatever the KEM, "key" and "base_nonce" with an encryption's "nonce", "aad", "pt" and "ct" are AES-GCM known
answers.  Kept per vector: kem_id, kdf_id, aead_id, mode, key, base_nonce, and of the 257 encryptions those at sequence numbers 0, 1,
2, 4, 255 and 256 (each with its "seq"; 256 is the first whose nonce differs from the base nonce in the second counter byte): 384
encryptions, 32 vectors with 16-byte keys and 32 with 32-byte keys.  Every pt is 29 bytes and every aad 7 - 9 bytes, so the file pins
the cipher, both key sizes and the sequence nonces, not lengths.  All binary fields are hex strings.
"""
import gzip
import json
import os

from make_golden_hpke import REF

OUT = os.path.dirname(os.path.abspath(__file__))
KEEP = ("kem_id", "kdf_id", "aead_id", "mode", "key", "base_nonce")
SEQS = (0, 1, 2, 4, 255, 256)


def main():
    with gzip.open(os.path.join(REF, "hpke/testdata/vectors_rfc9180_5f503c5.json.gz"), "rt") as f:
        vectors = json.load(f)
    data = []
    for v in vectors:
        if v["aead_id"] not in (1, 2):
            continue
        d = {k: v[k] for k in KEEP}
        d["encryptions"] = [dict({k: v["encryptions"][s][k] for k in ("nonce", "aad", "pt", "ct")}, seq=s) for s in SEQS]
        data.append(d)
    sizes = [len(d["key"]) // 2 for d in data]
    assert len(data) == 64 and sizes.count(16) == 32 and sizes.count(32) == 32 and all((s == 16) == (d["aead_id"] == 1) for s, d in zip(sizes, data))
    with gzip.GzipFile(os.path.join(OUT, "aesgcm_hpke.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("aesgcm_hpke.json.gz: %d vectors, %d encryptions" % (len(data), sum(len(d["encryptions"]) for d in data)))


if __name__ == "__main__":
    main()
