"""Builds and runs tests/prio3_test.cpp: the C++ mirror (include/circl/prio3.hpp) of the reference's prio3 Count and Sum over batches,
on the GPU.  The expected leader shares are the checker's (tests/prio3.py), handed to the program as hex arguments."""
import os
import subprocess

import pytest

import prio3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    from circl_amd import build as cbuild
    cbuild.build()
    out = os.path.join(ROOT, "build", "prio3_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "prio3_test.cpp"),
                           "-L", os.path.join(ROOT, "circl_amd"), "-lcirclhip", "-Wl,-rpath," + os.path.join(ROOT, "circl_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def pattern(n, a, b):
    """prio3_test.cpp pattern()"""
    return bytes((7 * j + 13 * a + b) & 0xFF for j in range(n))


def expected():
    """the program's arguments: per flow (Count, Sum with max_measurement 1000; three aggregators) the leader shares of its four reports"""
    out = []
    for kind, mx, meas in ((1, 0, (1, 0, 2, 1)), (2, 1000, (1000, 1001, 0, 337))):
        t = prio3.Task(kind, mx, 3, pattern(16, 0, 5))
        for i, m in enumerate(meas):
            try:
                out.append(t.shard(m, pattern(t.rand_size, i, 1)).hex())
            except prio3.Prio3Error:
                out.append("-")
    return out


def test_prio3_mirror_compiles():
    _build()
    e = expected()
    assert len(e) == 8 and e[2] == e[5] == "-" and len(e[0]) == 2 * 48


@pytest.mark.gpu
def test_prio3_mirror_runs():
    exe = _build()
    r = subprocess.run([exe] + expected(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
