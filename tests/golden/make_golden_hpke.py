#!/usr/bin/env python3
"""Writes tests/golden/hpke_dhkem.json.gz from the reference checkout (data only: the KEM-level fields of the RFC 9180 vectors
that hpke/vectors_test.go reads).  Run in the build container only (the GPU box has no reference checkout):
    python tests/golden/make_golden_hpke.py

From hpke/testdata/vectors_rfc9180_5f503c5.json.gz (1.7 MB, 128 vectors) the 64 vectors with kem_id 32 (DHKEM(X25519,
HKDF-SHA256)) or 33 (DHKEM(X448, HKDF-SHA512)): modes 0-3 (base, psk, auth, auth_psk), 8 of each per KEM.  Kept per vector: mode,
kem_id, ikmE / ikmR / ikmS, skEm / skRm / skSm, pkEm / pkRm / pkSm, enc, shared_secret (the S fields exist in modes 2 and 3
only).  The key schedule, AEAD and export fields are dropped.  All binary fields are hex strings.
"""
import gzip
import json
import os

REF = os.environ.get("CIRCL_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("mode", "kem_id", "ikmE", "ikmR", "ikmS", "skEm", "skRm", "skSm", "pkEm", "pkRm", "pkSm", "enc", "shared_secret")


def main():
    with gzip.open(os.path.join(REF, "hpke/testdata/vectors_rfc9180_5f503c5.json.gz"), "rt") as f:
        vectors = json.load(f)
    data = [{k: v[k] for k in FIELDS if k in v} for v in vectors if v["kem_id"] in (32, 33)]
    with gzip.GzipFile(os.path.join(OUT, "hpke_dhkem.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("hpke_dhkem.json.gz: %d vectors" % len(data))


if __name__ == "__main__":
    main()
