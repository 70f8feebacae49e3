"""Kyber768-X448 and Kyber1024-X448 at the C ABI without a device: the six size calls give the reference's sizes (kem/hybrid/
hybrid.go:123-157 over x448.Size = 56 and round-3 Kyber768 / Kyber1024), the next id is still unknown, and NULL arrays are refused."""
import os
import subprocess

import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {5: dict(seed=64, eseed=56, pk=56 + 1184, sk=56 + 2400, ct=56 + 1088, ss=56 + 32),
         6: dict(seed=64, eseed=56, pk=56 + 1568, sk=56 + 3168, ct=56 + 1568, ss=56 + 32)}


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


@pytest.mark.parametrize("scheme", [5, 6])
def test_sizes(L, scheme):
    got = {f: getattr(L, "circl_hip_hybrid_%s_size" % f)(scheme) for f in SIZES[scheme]}
    assert got == SIZES[scheme]
    assert got == {5: dict(seed=64, eseed=56, pk=1240, sk=2456, ct=1144, ss=88), 6: dict(seed=64, eseed=56, pk=1624, sk=3224, ct=1624, ss=88)}[scheme]
    # every row is a multiple of 8 bytes (the host pipeline's row alignment), and the workspace grows with n
    assert all(v % 8 == 0 for v in got.values())
    assert 0 < L.circl_hip_hybrid_workspace_size(scheme, 1) <= L.circl_hip_hybrid_workspace_size(scheme, 65)


def test_python_constants_and_table():
    from circl_amd import device, hostapi
    assert (hostapi.KYBER768_X448, hostapi.KYBER1024_X448) == (5, 6) == (device.KYBER768_X448, device.KYBER1024_X448)
    assert hostapi.HYBRID_SIZES[5] == SIZES[5] and hostapi.HYBRID_SIZES[6] == SIZES[6]
    assert callable(device.x448)


def test_the_next_id_is_still_unknown(L):
    for f in ("seed", "eseed", "pk", "sk", "ct", "ss"):
        assert getattr(L, "circl_hip_hybrid_%s_size" % f)(7) == 0
    assert L.circl_hip_hybrid_workspace_size(7, 1) == 0
    assert L.circl_hip_hybrid_keygen(7, None, None, None, 0, 0) == nat.EPARAM


@pytest.mark.parametrize("scheme", [5, 6])
def test_null_arrays_are_refused(L, scheme):
    import numpy as np
    buf = np.zeros(1 << 16, np.uint8)
    B = buf.ctypes.data
    assert L.circl_hip_hybrid_keygen(scheme, None, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_keygen(scheme, B, None, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_keygen(scheme, B, B, None, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_encaps(scheme, None, B, B, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_encaps(scheme, B, None, B, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_encaps(scheme, B, B, None, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_encaps(scheme, B, B, B, None, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_decaps(scheme, None, B, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_decaps(scheme, B, None, B, B, 1, 0) == nat.EPARAM
    assert L.circl_hip_hybrid_decaps(scheme, B, B, None, B, 1, 0) == nat.EPARAM


@pytest.mark.parametrize("scheme", [5, 6])
def test_no_key_table_for_the_x448_hybrids(L, scheme):
    import ctypes as C
    import numpy as np
    keys = np.zeros(4096, np.uint8)
    handle = C.c_void_p(1)
    for private in (0, 1):
        assert L.circl_hip_hybrid_keytable_new(scheme, private, keys.ctypes.data, 1, 0, None, C.byref(handle)) == nat.EPARAM
        assert not handle.value


def test_cpp_mirror_names_and_sizes(L, tmp_path):
    # include/circl/hybrid.hpp: Kyber768X448 / Kyber1024X448 carry the reference's names and sizes and agree with the library
    exe = str(tmp_path / "hybrid448_mirror_test")
    lib_dir = os.path.join(ROOT, "circl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hybrid448_mirror_test.cpp"),
                           "-o", exe, "-L", lib_dir, "-lcirclhip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hybrid448 mirror ok" in r.stdout, r.stdout + r.stderr
