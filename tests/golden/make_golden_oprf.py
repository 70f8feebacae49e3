#!/usr/bin/env python3
"""Writes tests/golden/oprf_ristretto255.json.gz from the reference checkout (data only).  Run where the reference is:
    CIRCL_REFERENCE=<checkout> python tests/golden/make_golden_oprf.py

  "rfc9497"   the three ristretto255-SHA512 entries (modes 0, 1, 2) of oprf/testdata/rfc9497.json.gz, whole: keys, blinds, blinded and
              evaluated elements, outputs and -- for the batch proofs that are not served yet -- the proofs
  "multiples" the 16 encodings 0 B .. 15 B of group/ristretto255_test.go (TestGeneratorMultiples)
  "invalid"   all 29 invalid encodings of TestInvalidEncodings as {"enc", "reference_accepts"}: the two that the reference comments out
              because it ignores bit 255 and reduces s >= p are included, flagged reference_accepts = true
  "scalars"   {"valid": 3, "invalid": 5} encodings of TestRistrettoScalarNonCanonical
The hex strings of the Go file are read as data: every quoted 64-digit string between a function's header and its closing brace.
"""
import gzip
import json
import os
import re
import sys

REF = os.environ.get("CIRCL_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else "")
OUT = os.path.dirname(os.path.abspath(__file__))
HEX = re.compile(r'^\s*(//\s*)?"([0-9a-f]{64})",\s*$')


def function_body(text, name):
    start = text.index("func %s(" % name)
    return text[start:text.index("\n}\n", start)]


def hex_lines(body, stop=None):
    """[(hex, commented_out)] in order, up to the line that holds `stop`"""
    out = []
    for line in body.splitlines():
        if stop and stop in line:
            break
        m = HEX.match(line)
        if m:
            out.append((m.group(2), bool(m.group(1))))
    return out


def main():
    if not REF:
        sys.exit("set CIRCL_REFERENCE to the reference checkout")
    with gzip.open(os.path.join(REF, "oprf/testdata/rfc9497.json.gz"), "rt") as f:
        rfc = [e for e in json.load(f) if e["identifier"] == "ristretto255-SHA512"]
    with open(os.path.join(REF, "group/ristretto255_test.go")) as f:
        go = f.read()
    multiples = [h for h, c in hex_lines(function_body(go, "TestGeneratorMultiples")) if not c]
    invalid = [{"enc": h, "reference_accepts": c} for h, c in hex_lines(function_body(go, "TestInvalidEncodings"))]
    body = function_body(go, "TestRistrettoScalarNonCanonical")
    valid = [h for h, _ in hex_lines(body, "invalid := []string{")]
    bad = [h for h, _ in hex_lines(body[body.index("invalid := []string{"):])]
    assert (len(rfc), len(multiples), len(invalid), len(valid), len(bad)) == (3, 16, 29, 3, 5)
    assert sum(e["reference_accepts"] for e in invalid) == 2
    data = {"rfc9497": rfc, "multiples": multiples, "invalid": invalid, "scalars": {"valid": valid, "invalid": bad}}
    with gzip.GzipFile(os.path.join(OUT, "oprf_ristretto255.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("oprf_ristretto255.json.gz: %d suites, %d items" % (len(rfc), sum(len(v["Input"].split(",")) for e in rfc for v in e["vectors"])))


if __name__ == "__main__":
    main()
