#!/usr/bin/env python3
"""Writes tests/golden/curve448.json.gz from the reference checkout (data only: the vectors that sign/ed448's and dh/x448's
own tests read).  Run in the build container only (the GPU box has no reference checkout):
    python tests/golden/make_golden_curve448.py

  wycheproof   sign/ed448/testdata/wycheproof_Ed448.json.gz (test logic: wycheproof_test.go), whole: 9 groups, 86 cases of
               which 17 are valid (they include the RFC 8032 7.4 vectors; messages up to 1023 bytes); sk (the group's seed),
               pk, msg, sig, valid (true only for result "valid"), tcId, comment.
  x448_kat     dh/x448/testdata/rfc7748_kat_test.json.gz, whole (6 cases): input (the point), scalar, output.
  x448_times   dh/x448/testdata/rfc7748_times_test.json.gz: the iterated vectors for 1 and 1000 iterations (10^6 is too slow for
               every side): times, key.
All binary fields are hex strings.
"""
import gzip
import json
import os

REF = os.environ.get("CIRCL_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    with gzip.open(os.path.join(REF, "sign/ed448/testdata/wycheproof_Ed448.json.gz"), "rt") as f:
        w = json.load(f)
    wyc = []
    for g in w["testGroups"]:
        for t in g["tests"]:
            wyc.append({"tcId": t["tcId"], "comment": t["comment"], "sk": g["key"]["sk"], "pk": g["key"]["pk"], "msg": t["msg"], "sig": t["sig"],
                        "valid": t["result"] == "valid"})
    with gzip.open(os.path.join(REF, "dh/x448/testdata/rfc7748_kat_test.json.gz"), "rt") as f:
        kat = [{"input": k["input"], "scalar": k["scalar"], "output": k["output"]} for k in json.load(f)]
    with gzip.open(os.path.join(REF, "dh/x448/testdata/rfc7748_times_test.json.gz"), "rt") as f:
        times = [{"times": k["times"], "key": k["key"]} for k in json.load(f) if k["times"] in (1, 1000)]
    data = {"wycheproof": wyc, "x448_kat": kat, "x448_times": times}
    with gzip.GzipFile(os.path.join(OUT, "curve448.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print("curve448.json.gz: %d Wycheproof cases, %d X448 KATs, %d iterated vectors" % (len(wyc), len(kat), len(times)))


if __name__ == "__main__":
    main()
