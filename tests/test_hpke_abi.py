"""CPU-side checks of the HPKE DHKEM and SHA-256 entry points of the C ABI: the size functions, the argument contract (checked before
any device is looked for) and, without a GPU, the loud failure of every compute call."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

OPS = {  # name -> (arguments after kem and before n, of which these may be NULL)
    "derive_keypair": (3, ()),
    "encap": (5, (4,)),
    "decap": (5, (1, 4)),
    "auth_encap": (7, (2, 6)),
    "auth_decap": (6, (1, 5)),
}


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def _buf(n=256):
    a = np.zeros(n, np.uint8)
    return a, a.ctypes.data_as(C.c_void_p)


def test_sizes(L):
    assert (L.circl_hip_hpke_dhkem_key_size(0x20), L.circl_hip_hpke_dhkem_ss_size(0x20)) == (32, 32)
    assert (L.circl_hip_hpke_dhkem_key_size(0x21), L.circl_hip_hpke_dhkem_ss_size(0x21)) == (56, 64)
    for kem in (0, 0x10, 0x12, 0x30, 0x22, -1):   # the P-curve KEMs and the hybrid one are not served
        assert L.circl_hip_hpke_dhkem_key_size(kem) == 0 and L.circl_hip_hpke_dhkem_ss_size(kem) == 0


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_argument_contract_before_any_device(L, op, suffix):
    nargs, optional = OPS[op]
    fn = getattr(L, "circl_hip_hpke_dhkem_" + op + suffix)
    keep, p = _buf()
    last = None if suffix else 0   # stream / device
    for kem in (0x20, 0x21):
        assert fn(kem, *([p] * nargs), 0, last) == nat.OK
        assert fn(kem, *([None] * nargs), 0, last) == nat.OK
        for j in range(nargs):
            args = [p] * nargs
            args[j] = None
            if j not in optional:
                assert fn(kem, *args, 1, last) == nat.EPARAM, (op, j)
    for kem in (0, 0x10, 0x30, 0x22):
        assert fn(kem, *([p] * nargs), 1, last) == nat.EPARAM
        assert fn(kem, *([p] * nargs), 0, last) == nat.EPARAM
    if suffix:   # a misaligned device pointer is refused before anything is launched
        for j in range(nargs):
            args = [p] * nargs
            args[j] = C.c_void_p(keep.ctypes.data + 1)
            if not (op != "derive_keypair" and j == nargs - 1):   # ok is a byte array
                assert fn(0x20, *args, 1, None) == nat.EWORKSPACE, (op, j)


def test_sha256_contract(L):
    keep, p = _buf()
    off = np.zeros(2, np.uint64)
    assert L.circl_hip_sha256(None, None, None, 0, 0) == nat.OK
    assert L.circl_hip_sha256(p, None, p, 1, 0) == nat.EPARAM
    assert L.circl_hip_sha256(p, off.ctypes.data_as(C.c_void_p), None, 1, 0) == nat.EPARAM


def test_no_gpu_means_loud_failure(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from circl_amd import hostapi as api
    for kem, N in ((0x20, 32), (0x21, 56)):
        z = np.zeros((2, N), np.uint8)
        for call in (lambda: api.hpke_dhkem_derive_keypair(kem, z), lambda: api.hpke_dhkem_encap(kem, z, z), lambda: api.hpke_dhkem_decap(kem, z, z),
                     lambda: api.hpke_dhkem_auth_encap(kem, z, z, z), lambda: api.hpke_dhkem_auth_decap(kem, z, z, z)):
            with pytest.raises(nat.CirclHipError) as e:
                call()
            assert e.value.code == nat.ENODEV
        keep, p = _buf()
        assert L.circl_hip_hpke_dhkem_encap_dev(kem, p, p, p, p, p, 1, None) == nat.ENODEV
    with pytest.raises(nat.CirclHipError) as e:
        api.sha256([b"abc"])
    assert e.value.code == nat.ENODEV
    with pytest.raises(ValueError):
        api.hpke_dhkem_encap(0x10, np.zeros((1, 65), np.uint8), np.zeros((1, 32), np.uint8))
