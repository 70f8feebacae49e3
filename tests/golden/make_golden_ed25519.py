#!/usr/bin/env python3
"""Writes tests/golden/ed25519.json.gz from the reference checkout (data only: the RFC 8032 and Wycheproof vectors that
sign/ed25519's own tests read).  Run in the build container only (the GPU box has no reference checkout):
    python tests/golden/make_golden_ed25519.py

  rfc8032      sign/ed25519/testdata/sign.input.txt.gz (test logic: rfc8032_test.go): lines 0-255 and every 8th line after
               (messages of 0..1023 bytes, so every SHA-512 block count up to nine); fields seed, pk, msg, sig.
  wycheproof   sign/ed25519/testdata/wycheproof_Ed25519.json.gz (test logic: wycheproof_test.go), whole: sk (the group's seed), pk, msg, sig, valid
               (true only for result "valid"), tcId, comment.
All binary fields are hex strings.
"""
import gzip
import json
import os

REF = os.environ.get("CIRCL_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    rfc = []
    with gzip.open(os.path.join(REF, "sign/ed25519/testdata/sign.input.txt.gz"), "rt") as f:
        for i, line in enumerate(f):
            if i >= 256 and i % 8:
                continue
            sk, pk, msg, sm = line.strip().split(":")[:4]
            rfc.append({"line": i, "seed": sk[:64], "pk": pk, "msg": msg, "sig": sm[:128]})
    with gzip.open(os.path.join(REF, "sign/ed25519/testdata/wycheproof_Ed25519.json.gz"), "rt") as f:
        w = json.load(f)
    wyc = []
    for g in w["testGroups"]:
        for t in g["tests"]:
            wyc.append({"tcId": t["tcId"], "comment": t["comment"], "sk": g["key"]["sk"], "pk": g["key"]["pk"], "msg": t["msg"], "sig": t["sig"],
                        "valid": t["result"] == "valid"})
    data = {"rfc8032": rfc, "wycheproof": wyc}
    with gzip.GzipFile(os.path.join(OUT, "ed25519.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("ed25519.json.gz: %d sign.input lines, %d Wycheproof cases" % (len(rfc), len(wyc)))


if __name__ == "__main__":
    main()
