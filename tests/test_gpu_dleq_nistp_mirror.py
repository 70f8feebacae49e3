"""Builds and runs tests/dleq_nistp_test.cpp: the C++ mirror (include/circl/oprf_nistp.hpp, namespace nistp::proofs) of the verifiable OPRF
modes on P-256 / P-384 -- VerifiableServer, PartialObliviousServer, VerifiableClient, PartialObliviousClient -- on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    from circl_amd import build as cbuild
    cbuild.build()
    out = os.path.join(ROOT, "build", "dleq_nistp_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dleq_nistp_test.cpp"),
                           "-L", os.path.join(ROOT, "circl_amd"), "-lcirclhip", "-Wl,-rpath," + os.path.join(ROOT, "circl_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_dleq_nistp_mirror_compiles():
    _build()


@pytest.mark.gpu
def test_dleq_nistp_mirror_runs():
    exe = _build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
