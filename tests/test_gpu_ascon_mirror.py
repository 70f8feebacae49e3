"""Builds and runs tests/ascon_test.cpp: the C++ mirror (include/circl/ascon.hpp) of cipher/ascon -- Mode and Cipher over batches -- on
the GPU.  The expected ciphertexts are the checker's (tests/ascon.py), handed to the program as hex arguments."""
import os
import subprocess

import pytest

import ascon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    from circl_amd import build as cbuild
    cbuild.build()
    out = os.path.join(ROOT, "build", "ascon_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ascon_test.cpp"),
                           "-L", os.path.join(ROOT, "circl_amd"), "-lcirclhip", "-Wl,-rpath," + os.path.join(ROOT, "circl_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def pattern(n, a, b):
    """ascon_test.cpp pattern()"""
    return bytes((7 * j + 13 * a + b) & 0xFF for j in range(n))


def expected():
    """the program's arguments: the TestAPI case, then three items per mode"""
    k16 = bytes(range(16))
    out = [ascon.seal(ascon.ASCON128, k16, k16, b"helloworld")]
    for m, mode in enumerate((ascon.ASCON128, ascon.ASCON128A, ascon.ASCON80PQ)):
        key = pattern(ascon.key_size(mode), m, 1)
        for i, (pl, al) in enumerate(zip((0, 9, 40), (5, 0, 17))):
            out.append(ascon.seal(mode, key, pattern(16, i, 2), pattern(pl, i, 3), pattern(al, i, 4)))
    return [x.hex() for x in out]


def test_ascon_mirror_compiles():
    _build()
    assert len(expected()) == 10 and len(expected()[0]) == 2 * 26


@pytest.mark.gpu
def test_ascon_mirror_runs():
    exe = _build()
    r = subprocess.run([exe] + expected(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
