"""CPU-side checks of the Ascon entry points of the C ABI: circl_hip_ascon_key_size and the argument contract, which is checked
before any device is looked for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure of every
well-formed call."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

KEEP = np.zeros(4096, np.uint8)
P = KEEP.ctypes.data_as(C.c_void_p)
OFF = np.zeros(8, np.uint64)
O = OFF.ctypes.data_as(C.c_void_p)

A128, A128A, A80PQ = 1, 2, -1
MODES = (A128, A128A, A80PQ)
ENTRY = {   # name -> its arguments before n, in order
    "seal": ["mode", "key", "key_stride", "nonce", "in", "pt_off", "aad", "aad_off", "out"],
    "open": ["mode", "key", "key_stride", "nonce", "in", "pt_off", "aad", "aad_off", "out", "ok"],
}
FORMS = [(e, s) for e in ENTRY for s in ("", "_dev")]


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def call(lib, entry, suffix, n=1, **over):
    """the entry point with well-formed arguments (Ascon128, one key for the batch), except for `over`"""
    args = []
    for a in ENTRY[entry]:
        if a in over:
            v = over[a]
        elif a == "mode":
            v = A128
        elif a == "key_stride":
            v = 0
        else:
            v = O if a.endswith("_off") else P
        args.append(v)
    return getattr(lib, "circl_hip_ascon_" + entry + suffix)(*args, n, None if suffix else 0)


def test_key_size(L):
    assert [L.circl_hip_ascon_key_size(m) for m in MODES] == [16, 16, 20]
    assert [L.circl_hip_ascon_key_size(m) for m in (0, 3, -2, 4, 255)] == [0] * 5


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    for mode in MODES:
        ks = L.circl_hip_ascon_key_size(mode)
        for stride in (0, ks, 32, 64):
            assert call(L, entry, suffix, n=0, mode=mode, key_stride=stride) == nat.OK
            if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
                assert call(L, entry, suffix, mode=mode, key_stride=stride) == nat.ENODEV
    if _no_gpu():
        assert call(L, entry, suffix, aad=None, aad_off=None) == nat.ENODEV
        assert call(L, entry, suffix, aad=None) == nat.ENODEV                    # offsets without a blob: not read
        if entry == "open":
            assert call(L, entry, suffix, pt_off=None) == nat.ENODEV             # rows of tags
            assert call(L, entry, suffix, ok=None) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_unknown_modes(L, entry, suffix):
    for n in (0, 1):
        for mode in (0, 3, -2):
            assert call(L, entry, suffix, n, mode=mode) == nat.EPARAM, mode


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_key_strides(L, entry, suffix):
    for n in (0, 1):
        for mode, stride in ((A128, 4), (A128A, 4), (A80PQ, 4), (A80PQ, 16), (A80PQ, 18), (A128, 15), (A128, 18), (A128A, 12), (A80PQ, 22)):
            assert call(L, entry, suffix, n, mode=mode, key_stride=stride) == nat.EPARAM, (mode, stride)


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_required_pointers_and_blobs(L, entry, suffix):
    for k in ("key", "nonce", "out"):
        assert call(L, entry, suffix, **{k: None}) == nat.EPARAM, k
        assert call(L, entry, suffix, 0, **{k: None}) == nat.OK
    assert call(L, entry, suffix, aad=P, aad_off=None) == nat.EPARAM             # an aad blob without offsets
    if entry == "seal":
        assert call(L, entry, suffix, pt_off=None) == nat.EPARAM                 # a plaintext blob without offsets
        assert call(L, entry, suffix, 0, **{"in": None, "pt_off": None}) == nat.OK
        if _no_gpu():
            assert call(L, entry, suffix, **{"in": None, "pt_off": None}) == nat.ENODEV   # every plaintext is empty
    else:
        assert call(L, entry, suffix, **{"in": None}) == nat.EPARAM              # a ciphertext always has its tags
        assert call(L, entry, suffix, **{"in": None, "pt_off": None}) == nat.EPARAM


def test_misaligned_device_pointers(L):
    odd = C.c_void_p(KEEP.ctypes.data + 2)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    for entry in ENTRY:
        assert call(L, entry, "_dev", key=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", nonce=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", pt_off=odd4) == nat.EWORKSPACE
        assert call(L, entry, "_dev", aad_off=odd4) == nat.EWORKSPACE
        assert call(L, entry, "_dev", key=odd, mode=0) == nat.EPARAM             # the contract comes first


def test_no_gpu_means_loud_failure(L):
    from circl_amd import hostapi as api
    for mode, ks in ((A128, 16), (A128A, 16), (A80PQ, 20)):
        c = api.AsconCipher(mode, bytes(ks))
        assert (c.key_size, c.nonce_size, c.overhead) == (ks, 16, 16)
        nonces = np.zeros((2, 16), np.uint8)
        if _no_gpu():
            for f in (lambda: c.seal(nonces, [b"a", b""]), lambda: c.open(nonces, [bytes(16), bytes(17)], [b"x", b""])):
                with pytest.raises(nat.CirclHipError) as e:
                    f()
                assert e.value.code == nat.ENODEV
        with pytest.raises(ValueError):
            api.AsconCipher(mode, bytes(ks + 1))
        with pytest.raises(ValueError):
            c.open(nonces, [bytes(16), bytes(15)])
    with pytest.raises(ValueError):
        api.AsconCipher(0, bytes(16))
