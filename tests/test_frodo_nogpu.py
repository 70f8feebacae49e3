"""FrodoKEM-640-SHAKE bindings without a GPU: wrong row lengths are refused before anything is launched, the workspace size is
what the header says, and where there is no device every new call says so (CIRCL_HIP_ENODEV) instead of computing anything."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import hostapi

PK, SK, CT = 9616, 19888, 9720


def test_wrong_row_lengths_are_refused():
    z = lambda n, c: np.zeros((n, c), np.uint8)  # noqa: E731
    for call in (lambda: hostapi.frodo640shake_keygen(z(1, 47)),
                 lambda: hostapi.frodo640shake_keygen(bytes(49)),
                 lambda: hostapi.frodo640shake_keygen([bytes(48), bytes(47)]),
                 lambda: hostapi.frodo640shake_keygen(np.zeros(96, np.uint8)),           # flat: not rows
                 lambda: hostapi.frodo640shake_encaps(z(1, PK - 1), z(1, 16)),
                 lambda: hostapi.frodo640shake_encaps(z(2, PK // 2), z(2, 16)),          # the right number of bytes in the wrong rows
                 lambda: hostapi.frodo640shake_encaps(z(1, PK), z(1, 32)),
                 lambda: hostapi.frodo640shake_encaps(z(2, PK), z(1, 16)),
                 lambda: hostapi.frodo640shake_decaps(z(1, SK), z(1, CT + 1)),
                 lambda: hostapi.frodo640shake_decaps(z(1, SK - 16), z(1, CT)),
                 lambda: hostapi.frodo640shake_decaps(z(1, SK), z(2, CT))):
        with pytest.raises(ValueError):
            call()
    assert hostapi.FRODO640SHAKE_SIZES == dict(pk=PK, sk=SK, ct=CT, ss=16, seed=48, eseed=16)


def test_workspace_size_is_monotone():
    L = nat.lib()
    sizes = [L.circl_hip_frodo640shake_workspace_size(n) for n in (0, 1, 2, 63, 64, 65, 1000, 1 << 16)]
    assert sizes[0] == 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    assert sizes[1] >= 20608 + 16 + 16 + CT and sizes[-1] >= (1 << 16) * (20608 + 32 + CT)


def test_no_device_is_said_so():
    import torch
    if torch.cuda.is_available():
        return  # on a GPU machine tests/test_gpu_frodo.py covers the calls
    L = nat.lib()
    buf = np.zeros(2 * SK, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.circl_hip_frodo640shake_keygen(p, p, p, 1, 0) == nat.ENODEV
    assert L.circl_hip_frodo640shake_encaps(p, p, p, p, 1, 0) == nat.ENODEV
    assert L.circl_hip_frodo640shake_decaps(p, p, p, 1, -1) == nat.ENODEV
    assert L.circl_hip_frodo640shake_keygen_dev(p, p, p, 1, p, 1 << 20, None) == nat.ENODEV
    assert L.circl_hip_frodo640shake_encaps_dev(p, p, p, p, 1, p, 1 << 20, None) == nat.ENODEV
    assert L.circl_hip_frodo640shake_decaps_dev(p, p, p, 1, p, 1 << 20, None) == nat.ENODEV
    for call in (lambda: hostapi.frodo640shake_keygen(np.zeros((1, 48), np.uint8)),
                 lambda: hostapi.frodo640shake_encaps(np.zeros((1, PK), np.uint8), np.zeros((1, 16), np.uint8)),
                 lambda: hostapi.frodo640shake_decaps(np.zeros((1, SK), np.uint8), np.zeros((1, CT), np.uint8))):
        with pytest.raises(nat.CirclHipError) as e:
            call()
        assert e.value.code == nat.ENODEV
