"""Builds and runs tests/aesgcm_test.cpp: the C++ mirror (include/circl/aesgcm.hpp) of cipher.AEAD for AES-GCM over batches, on the
GPU.  The expected ciphertexts are the checker's (tests/aesgcm.py), handed to the program as hex arguments."""
import os
import subprocess

import pytest

import aesgcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    from circl_amd import build as cbuild
    cbuild.build()
    out = os.path.join(ROOT, "build", "aesgcm_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "aesgcm_test.cpp"),
                           "-L", os.path.join(ROOT, "circl_amd"), "-lcirclhip", "-Wl,-rpath," + os.path.join(ROOT, "circl_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def pattern(n, a, b):
    """aesgcm_test.cpp pattern()"""
    return bytes((7 * j + 13 * a + b) & 0xFF for j in range(n))


def expected():
    """the program's arguments: per key size three items under explicit nonces, then three under base nonce + seq 255 + i"""
    out = []
    for k, ks in enumerate(aesgcm.KEY_SIZES):
        key = pattern(ks, k, 1)
        items = [(pattern(pl, i, 3), pattern(al, i, 4)) for i, (pl, al) in enumerate(zip((0, 9, 40), (5, 0, 17)))]
        out += [aesgcm.seal(key, pattern(12, i, 2), pt, ad) for i, (pt, ad) in enumerate(items)]
        out += [aesgcm.seal(key, aesgcm.seq_nonce(pattern(12, 0, 2), 255 + i), pt, ad) for i, (pt, ad) in enumerate(items)]
    return [x.hex() for x in out]


def test_aesgcm_mirror_compiles():
    _build()
    assert len(expected()) == 12 and len(expected()[0]) == 2 * 16


@pytest.mark.gpu
def test_aesgcm_mirror_runs():
    exe = _build()
    r = subprocess.run([exe] + expected(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
