#!/usr/bin/env python3
"""Writes tests/golden/ascon.json.gz from the reference checkout (data only: the known-answer vectors that cipher/ascon/ascon_test.go
reads).  Run in the build container only (the GPU box has no reference checkout):
    python tests/golden/make_golden_ascon.py

All 1089 vectors of each of cipher/ascon/testdata/{Ascon128,Ascon128a,Ascon80pq}.json.gz: every pair of a plaintext and an
associated-data length in 0..32.  Every vector of a mode has the same key and the same nonce, so the file keeps them once per mode:
    {"Ascon128": {"Key": hex, "Nonce": hex, "vectors": [{"PT": hex, "AD": hex, "CT": hex}, ...]}, ...}
CT is ciphertext || tag.
"""
import gzip
import json
import os

from make_golden_hpke import REF

OUT = os.path.dirname(os.path.abspath(__file__))
MODES = ("Ascon128", "Ascon128a", "Ascon80pq")


def main():
    data = {}
    for m in MODES:
        with gzip.open(os.path.join(REF, "cipher/ascon/testdata/%s.json.gz" % m), "rt") as f:
            vectors = json.load(f)
        key, nonce = vectors[0]["Key"], vectors[0]["Nonce"]
        assert all(v["Key"] == key and v["Nonce"] == nonce for v in vectors)
        data[m] = {"Key": key, "Nonce": nonce, "vectors": [{k: v[k] for k in ("PT", "AD", "CT")} for v in vectors]}
    with gzip.GzipFile(os.path.join(OUT, "ascon.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("ascon.json.gz: " + ", ".join("%s %d" % (m, len(data[m]["vectors"])) for m in MODES))


if __name__ == "__main__":
    main()
