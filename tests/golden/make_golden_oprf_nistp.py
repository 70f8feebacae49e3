#!/usr/bin/env python3
"""Writes tests/golden/oprf_nistp.json.gz from the reference checkout (data only).  Run where the reference is:
    CIRCL_REFERENCE=<checkout> python tests/golden/make_golden_oprf_nistp.py

  "rfc9497"  the six P256-SHA256 / P384-SHA384 entries (modes 0, 1, 2 each) of oprf/testdata/rfc9497.json.gz, whole: keys, blinds,
             blinded and evaluated elements, outputs and -- for the proofs that are not served on these curves -- the proofs
  "h2c"      the four hash-to-curve files group/testdata/P{256,384}_XMD-SHA-{256,384}_SSWU_{RO,NU}_.json.gz, whole, keyed by
             "P256_RO", "P256_NU", "P384_RO", "P384_NU": five messages each with u, Q0 / Q1 or Q, and P
"""
import gzip
import json
import os
import sys

REF = os.environ.get("CIRCL_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else "")
OUT = os.path.dirname(os.path.abspath(__file__))
SUITES = ("P256-SHA256", "P384-SHA384")
H2C = {"P256_RO": "P256_XMD-SHA-256_SSWU_RO_", "P256_NU": "P256_XMD-SHA-256_SSWU_NU_",
       "P384_RO": "P384_XMD-SHA-384_SSWU_RO_", "P384_NU": "P384_XMD-SHA-384_SSWU_NU_"}


def main():
    if not REF:
        sys.exit("set CIRCL_REFERENCE to the reference checkout")
    with gzip.open(os.path.join(REF, "oprf/testdata/rfc9497.json.gz"), "rt") as f:
        rfc = [e for e in json.load(f) if e["identifier"] in SUITES]
    assert [(e["identifier"], e["mode"]) for e in rfc] == [(s, m) for s in SUITES for m in (0, 1, 2)]
    h2c = {}
    for key, name in H2C.items():
        with gzip.open(os.path.join(REF, "group/testdata", name + ".json.gz"), "rt") as f:
            h2c[key] = json.load(f)
        assert [len(v["msg"]) for v in h2c[key]["vectors"]] == [0, 3, 16, 133, 517]
    with gzip.GzipFile(os.path.join(OUT, "oprf_nistp.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps({"rfc9497": rfc, "h2c": h2c}, separators=(",", ":")).encode())
    print("oprf_nistp.json.gz: %d suites, %d items, %d hash-to-curve vectors" %
          (len(rfc), sum(len(v["Input"].split(",")) for e in rfc for v in e["vectors"]), sum(len(h["vectors"]) for h in h2c.values())))


if __name__ == "__main__":
    main()
