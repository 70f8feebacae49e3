"""Builds and runs tests/dleq_test.cpp: the C++ mirror (include/circl/oprf.hpp) of the verifiable modes -- VerifiableServer / VerifiableClient,
PartialObliviousServer / PartialObliviousClient -- on the GPU, on the batch-of-two RFC 9497 vectors of modes 1 and 2."""
import os
import subprocess

import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("oprf_ristretto255.json.gz")


def _build():
    from circl_amd import build as cbuild
    cbuild.build()
    out = os.path.join(ROOT, "build", "dleq_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dleq_test.cpp"),
                           "-L", os.path.join(ROOT, "circl_amd"), "-lcirclhip", "-Wl,-rpath," + os.path.join(ROOT, "circl_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_dleq_mirror_compiles():
    _build()


@pytest.mark.gpu
def test_dleq_mirror_runs():
    exe = _build()
    v1, v2 = G["rfc9497"][1]["vectors"][2], G["rfc9497"][2]["vectors"][2]
    assert v1["Blind"] == v2["Blind"]
    r = subprocess.run([exe, v1["Proof"]["r"], v2["Proof"]["r"], *v1["Blind"].split(",")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    got = [line.split() for line in r.stdout.splitlines()[:-1]]
    want = [["proof1", v1["Proof"]["proof"]]] + [["out1", o] for o in v1["Output"].split(",")] + \
           [["proof2", v2["Proof"]["proof"]]] + [["out2", o] for o in v2["Output"].split(",")]
    assert got == want
