"""Writes tests/golden/prio3.json.gz from the reference's vdaf/prio3/testdata: the six Prio3Count / Prio3Sum vector files (the task's
parameters and, per report, measurement, nonce, rand, input shares, prep shares, out shares; agg_shares and agg_result) and the
XofTurboShake128 vector.  Data only; run once where the reference is at hand:

    python tests/golden/make_golden_prio3.py <reference>/vdaf/prio3/testdata
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ["Prio3Count_0", "Prio3Count_1", "Prio3Count_2", "Prio3Sum_0", "Prio3Sum_1", "Prio3Sum_2"]


def load(d, name):
    with gzip.open(os.path.join(d, name + ".json.gz")) as f:
        return json.load(f)


def main(d):
    out = {"files": {}, "xof": load(d, "XofTurboShake128")}
    for name in FILES:
        v = load(d, name)
        out["files"][name] = {
            "kind": 1 if "Count" in name else 2,
            "max_measurement": v.get("max_measurement", 0),
            "shares": v["shares"],
            "ctx": v["ctx"],
            "verify_key": v["verify_key"],
            "agg_shares": v["agg_shares"],
            "agg_result": v["agg_result"],
            "prep": [{k: p[k] for k in ("measurement", "nonce", "rand", "input_shares", "prep_shares", "out_shares")} for p in v["prep"]],
        }
    with gzip.GzipFile(os.path.join(HERE, "prio3.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode())


if __name__ == "__main__":
    main(sys.argv[1])
