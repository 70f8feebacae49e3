"""CPU-side checks of the AES-GCM entry points of the C ABI: the argument contract, which is checked before any device is looked for
(so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure of every well-formed call.  The HPKE
entry points still refuse the AES-GCM suites: wiring them is a later change."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

KEEP = np.zeros(4096, np.uint8)
P = KEEP.ctypes.data_as(C.c_void_p)
OFF = np.zeros(8, np.uint64)
O = OFF.ctypes.data_as(C.c_void_p)

SIZES = (16, 32)
ENTRY = {   # name -> its arguments before n, in order
    "seal": ["key_bytes", "key", "key_stride", "nonce", "nonce_stride", "seq", "in", "pt_off", "aad", "aad_off", "out"],
    "open": ["key_bytes", "key", "key_stride", "nonce", "nonce_stride", "seq", "in", "pt_off", "aad", "aad_off", "out", "ok"],
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
    """the entry point with well-formed arguments (AES-128-GCM, one key for the batch, nonce rows of 12, no seq), except for `over`"""
    args = []
    for a in ENTRY[entry]:
        if a in over:
            v = over[a]
        elif a == "key_bytes":
            v = 16
        elif a == "key_stride":
            v = 0
        elif a == "nonce_stride":
            v = 12
        elif a == "seq":
            v = None
        else:
            v = O if a.endswith("_off") else P
        args.append(v)
    return getattr(lib, "circl_hip_aesgcm_" + entry + suffix)(*args, n, None if suffix else 0)


def test_the_constants_and_the_kernel_ids():
    import os
    import re
    with open(os.path.join(cbuild.ROOT, "include", "circl_hip.h")) as f:
        h = f.read()
    d = dict(re.findall(r"#define (CIRCL_HIP_\w+) (\d+)", h))
    assert (d["CIRCL_HIP_AES128GCM"], d["CIRCL_HIP_AES256GCM"]) == ("16", "32")
    assert (d["CIRCL_HIP_KERNEL_AESGCM_SEAL"], d["CIRCL_HIP_KERNEL_AESGCM_OPEN"], d["CIRCL_HIP_KERNEL_COUNT"]) == ("44", "45", "46")


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    for kb in SIZES:
        for stride in (0, kb, kb + 4, 80, 112):
            for nstride, seq in ((12, None), (16, None), (80, None), (12, O), (0, O), (112, O)):
                kw = dict(key_bytes=kb, key_stride=stride, nonce_stride=nstride, seq=seq)
                assert call(L, entry, suffix, n=0, **kw) == nat.OK
                if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
                    assert call(L, entry, suffix, **kw) == nat.ENODEV
    if _no_gpu():
        assert call(L, entry, suffix, aad=None, aad_off=None) == nat.ENODEV
        assert call(L, entry, suffix, aad=None) == nat.ENODEV                    # offsets without a blob: not read
        if entry == "open":
            assert call(L, entry, suffix, pt_off=None) == nat.ENODEV             # rows of tags
            assert call(L, entry, suffix, ok=None) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_key_sizes(L, entry, suffix):
    for n in (0, 1):
        for kb in (24, 0, -16, 1, 8, 15, 17, 31, 33, 48, 64, 128, 256):
            assert call(L, entry, suffix, n, key_bytes=kb) == nat.EPARAM, kb
            assert call(L, entry, suffix, n, key_bytes=kb, key_stride=64) == nat.EPARAM, kb


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_key_strides(L, entry, suffix):
    for n in (0, 1):
        for kb, stride in ((16, 4), (16, 12), (16, 15), (16, 18), (32, 16), (32, 28), (32, 30), (32, 34), (16, 81)):
            assert call(L, entry, suffix, n, key_bytes=kb, key_stride=stride) == nat.EPARAM, (kb, stride)


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_nonce_strides(L, entry, suffix):
    for n in (0, 1):
        for stride in (4, 8, 11, 13, 14, 18, 81):
            for seq in (None, O):
                assert call(L, entry, suffix, n, nonce_stride=stride, seq=seq) == nat.EPARAM, (stride, seq)
        assert call(L, entry, suffix, n, nonce_stride=0) == nat.EPARAM               # one base nonce for the batch needs seq
    assert call(L, entry, suffix, 0, nonce_stride=0, seq=O) == nat.OK


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


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_the_host_forms_refuse_a_plaintext_that_is_too_long(L, entry):
    """2^36 - 32 bytes is the most; the host forms read the offsets (nothing of the blob is touched before the refusal)"""
    limit = (1 << 36) - 32
    for lens, rc in (([limit + 1], nat.EPARAM), ([5, limit + 1], nat.EPARAM), ([1 << 40], nat.EPARAM)):
        off = np.concatenate([[0], np.cumsum(np.array(lens, np.uint64))]).astype(np.uint64)
        assert call(L, entry, "", len(lens), pt_off=off.ctypes.data_as(C.c_void_p)) == rc, lens
    down = np.array([8, 4], np.uint64)                                            # offsets that go down
    assert call(L, entry, "", 1, pt_off=down.ctypes.data_as(C.c_void_p)) == nat.EPARAM
    if _no_gpu():
        ok = np.array([0, limit], np.uint64)
        assert call(L, entry, "", 1, pt_off=ok.ctypes.data_as(C.c_void_p)) == nat.ENODEV


def test_misaligned_device_pointers(L):
    odd = C.c_void_p(KEEP.ctypes.data + 2)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    for entry in ENTRY:
        assert call(L, entry, "_dev", key=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", nonce=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", pt_off=odd4) == nat.EWORKSPACE
        assert call(L, entry, "_dev", aad_off=odd4) == nat.EWORKSPACE
        assert call(L, entry, "_dev", seq=odd4) == nat.EWORKSPACE
        assert call(L, entry, "_dev", key=odd, key_bytes=24) == nat.EPARAM       # the contract comes first


def test_no_gpu_means_loud_failure(L):
    from circl_amd import hostapi as api
    for ks in SIZES:
        c = api.AesGcm(bytes(ks))
        assert (c.key_size, c.nonce_size, c.overhead) == (ks, 12, 16)
        nonces = np.zeros((2, 12), np.uint8)
        if _no_gpu():
            for f in (lambda: c.seal(nonces, [b"a", b""]), lambda: c.open(nonces, [bytes(16), bytes(17)], [b"x", b""]),
                      lambda: c.seal(bytes(12), [b"a", b""], seq=[0, 1])):
                with pytest.raises(nat.CirclHipError) as e:
                    f()
                assert e.value.code == nat.ENODEV
        with pytest.raises(ValueError):
            c.open(nonces, [bytes(16), bytes(15)])
        with pytest.raises(ValueError):
            c.seal(nonces, [b"a"])
    for bad in (0, 15, 24, 33):
        with pytest.raises(ValueError):
            api.AesGcm(bytes(bad))


def test_the_hpke_entry_points_still_refuse_aes_gcm(L):
    """aead = 1 (AES-128-GCM) and 2 (AES-256-GCM) stay out of the HPKE entry points in this change"""
    for aead in (1, 2):
        for suffix in ("", "_dev"):
            seal = getattr(L, "circl_hip_hpke_seal" + suffix)
            for n in (0, 1):
                assert seal(aead, P, 112, O, P, O, P, O, P, n, None if suffix else 0) == nat.EPARAM, (aead, suffix, n)
    assert L.circl_hip_hpke_seal(3, P, 112, O, P, O, P, O, P, 0, 0) == nat.OK      # (the same call under ChaCha20-Poly1305 is well formed)
