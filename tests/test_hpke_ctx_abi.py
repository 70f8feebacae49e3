"""CPU-side checks of the HPKE context entry points of the C ABI: circl_hip_hpke_context_size and the argument contract, which is
checked before any device is looked for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure
of every well-formed call."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

KEEP = np.zeros(4096, np.uint8)
P = KEEP.ctypes.data_as(C.c_void_p)
OFF = np.zeros(8, np.uint64)
O = OFF.ctypes.data_as(C.c_void_p)

SENDER = ["kem", "kdf", "aead", "mode", "pkR", "ikmE", "skS", "pkS", "info", "info_off", "psk", "psk_off", "psk_id", "psk_id_off"]
RECEIVER = ["kem", "kdf", "aead", "mode", "skR", "pkR", "enc_in", "pkS", "info", "info_off", "psk", "psk_off", "psk_id", "psk_id_off"]
AEAD_IN = ["in", "pt_off", "aad", "aad_off"]
ENTRY = {   # name -> its arguments before n, in order
    "setup_sender": SENDER + ["enc", "ctx", "ok"],
    "setup_receiver": RECEIVER + ["ctx", "ok"],
    "seal": ["aead", "ctx", "ctx_stride", "seq"] + AEAD_IN + ["out"],
    "open": ["aead", "ctx", "ctx_stride", "seq"] + AEAD_IN + ["out", "ok"],
    "export": ["kdf", "kem", "aead", "ctx", "ctx_stride", "exp", "exp_off", "L", "out"],
    "seal_single": SENDER + AEAD_IN + ["enc", "out", "ok"],
    "open_single": RECEIVER + AEAD_IN + ["out", "ok"],
    "export_single": SENDER + ["exp", "exp_off", "L", "enc", "out", "ok"],
    "export_single_receiver": RECEIVER + ["exp", "exp_off", "L", "out", "ok"],
}
SETUPS = [e for e in ENTRY if "mode" in ENTRY[e]]
SCALARS = dict(kem=0x20, kdf=1, aead=3, mode=0, ctx_stride=112, L=32)
NULL_IN_BASE_MODE = ("skS", "pkS", "psk", "psk_off", "psk_id", "psk_id_off")
FORMS = [(e, s) for e in ENTRY for s in ("", "_dev")]


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def call(lib, entry, suffix, n=1, **over):
    """the entry point with well-formed mode-0 arguments, except for `over`"""
    args = []
    for a in ENTRY[entry]:
        if a in over:
            v = over[a]
        elif a in SCALARS:
            v = SCALARS[a]
        elif a in NULL_IN_BASE_MODE:
            v = None
        else:
            v = O if a.endswith("_off") or a == "seq" else P
        args.append(v)
    return getattr(lib, "circl_hip_hpke_" + entry + suffix)(*args, n, None if suffix else 0)


def well_formed(rc):
    """what a call that passes the contract returns here: it never ran (n = 0) or found no device"""
    return rc in (nat.OK, nat.ENODEV)


def test_context_size(L):
    assert [L.circl_hip_hpke_context_size(k) for k in (1, 3)] == [80, 112]
    assert [L.circl_hip_hpke_context_size(k) for k in (0, 2, 4, 0xFFFF, -1)] == [0] * 5


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    assert call(L, entry, suffix, n=0) == nat.OK
    if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
        assert call(L, entry, suffix) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_out_of_scope_suites(L, entry, suffix):
    names = ENTRY[entry]
    for n in (0, 1):
        if "kem" in names:
            for kem in (0x10, 0x11, 0x12, 0x30, 0x22, 0):          # P-256, P-384, P-521, X25519Kyber768, unassigned
                assert call(L, entry, suffix, n, kem=kem) == nat.EPARAM, kem
        if "kdf" in names:
            for kdf in (2, 0, 4):                                  # HKDF-SHA384
                assert call(L, entry, suffix, n, kdf=kdf) == nat.EPARAM, kdf
        for aead in (1, 2, 0, 4):                                  # AES-128-GCM, AES-256-GCM
            assert call(L, entry, suffix, n, aead=aead) == nat.EPARAM, aead
        if "mode" in names:
            for mode in (4, 5, -1, 255):
                assert call(L, entry, suffix, n, mode=mode) == nat.EPARAM, mode


@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_seal_and_open_refuse_the_export_only_aead(L, suffix):
    for entry in ("seal", "open", "seal_single", "open_single"):
        assert call(L, entry, suffix, aead=0xFFFF) == nat.EPARAM
        assert call(L, entry, suffix, n=0, aead=0xFFFF) == nat.EPARAM
    for entry in ("setup_sender", "setup_receiver", "export", "export_single", "export_single_receiver"):
        assert call(L, entry, suffix, n=0, aead=0xFFFF) == nat.OK


@pytest.mark.parametrize("entry", SETUPS)
@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_keys_and_psk_against_the_mode(L, entry, suffix):
    sender = "ikmE" in ENTRY[entry]
    psk = dict(psk=P, psk_off=O, psk_id=P, psk_id_off=O)
    auth = dict(skS=P, pkS=P) if sender else dict(pkS=P)
    ok = lambda **kw: well_formed(call(L, entry, suffix, 1 if _no_gpu() else 0, **kw))    # (with a GPU these host pointers must not reach a kernel)
    bad = lambda **kw: call(L, entry, suffix, **kw) == nat.EPARAM
    # the psk blobs: NULL in modes 0 and 2
    for mode, extra in ((0, {}), (2, auth)):
        assert ok(mode=mode, **extra)
        assert bad(mode=mode, **extra, **psk) and bad(mode=mode, **extra, psk=P, psk_off=O) and bad(mode=mode, **extra, psk_id=P, psk_id_off=O)
    for mode, extra in ((1, {}), (3, auth)):
        assert ok(mode=mode, **extra, **psk)
        assert ok(mode=mode, **extra)                                 # no blob: every item fails the psk rule, by its mask
        assert bad(mode=mode, **extra, psk=P, psk_off=None) and bad(mode=mode, **extra, **dict(psk, psk_id_off=None))
    # the sender's key pair / the sender's public key: NULL in modes 0 and 1, required in modes 2 and 3
    for mode, extra in ((0, {}), (1, psk)):
        for k in auth:
            assert bad(mode=mode, **extra, **{k: P})
    for mode, extra in ((2, {}), (3, psk)):
        assert bad(mode=mode, **extra)
        for k in auth:
            assert bad(mode=mode, **extra, **{j: P for j in auth if j != k})
    # what every mode needs
    for k in (("pkR", "ikmE", "enc") if sender else ("skR", "enc_in")):
        assert bad(**{k: None})
    if not sender:
        assert ok(pkR=None)                                              # the receiver's own public key is optional
    assert bad(info=P, info_off=None)
    assert ok(info=None, info_off=None)


@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_export_lengths(L, suffix):
    for entry in ("export", "export_single", "export_single_receiver"):
        for kdf, nh in ((1, 32), (3, 64)):
            for n in (0, 1):
                assert call(L, entry, suffix, n, kdf=kdf, L=0) == nat.EPARAM
                assert call(L, entry, suffix, n, kdf=kdf, L=255 * nh + 1) == nat.EPARAM
            assert call(L, entry, suffix, 0, kdf=kdf, L=255 * nh) == nat.OK
            assert call(L, entry, suffix, 0, kdf=kdf, L=1) == nat.OK
        assert call(L, entry, suffix, out=None) == nat.EPARAM
        assert call(L, entry, suffix, exp=P, exp_off=None) == nat.EPARAM


@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_rows_and_blobs(L, suffix):
    for entry in ("seal", "open", "export"):
        assert call(L, entry, suffix, ctx=None) == nat.EPARAM
        for stride in (0, 44, 50, 81):
            assert call(L, entry, suffix, ctx_stride=stride) == nat.EPARAM, (entry, stride)
    assert call(L, "export", suffix, kdf=3, ctx_stride=80) == nat.EPARAM     # shorter than a SHA-512 context
    assert call(L, "export", suffix, 0, kdf=1, ctx_stride=80) == nat.OK
    assert call(L, "seal", suffix, 0, ctx_stride=48) == nat.OK
    for entry in ("seal", "open", "seal_single", "open_single"):
        assert call(L, entry, suffix, out=None) == nat.EPARAM
        assert call(L, entry, suffix, aad=P, aad_off=None) == nat.EPARAM
    for entry in ("seal", "seal_single"):
        assert call(L, entry, suffix, pt_off=None) == nat.EPARAM          # a plaintext blob without offsets
        assert call(L, entry, suffix, 0, **{"in": None, "pt_off": None}) == nat.OK
    for entry in ("open", "open_single"):
        assert call(L, entry, suffix, **{"in": None}) == nat.EPARAM       # a ciphertext always has its tags
    assert call(L, "setup_sender", suffix, ctx=None) == nat.EPARAM and call(L, "setup_receiver", suffix, ctx=None) == nat.EPARAM


def test_misaligned_device_pointers(L):
    odd = C.c_void_p(KEEP.ctypes.data + 1)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    assert call(L, "setup_sender", "_dev", pkR=odd) == nat.EWORKSPACE
    assert call(L, "setup_receiver", "_dev", ctx=odd) == nat.EWORKSPACE
    assert call(L, "seal", "_dev", ctx=odd) == nat.EWORKSPACE
    assert call(L, "seal", "_dev", seq=odd4) == nat.EWORKSPACE
    assert call(L, "open", "_dev", pt_off=odd4) == nat.EWORKSPACE
    assert call(L, "export", "_dev", exp_off=odd4) == nat.EWORKSPACE


def test_no_gpu_means_loud_failure():
    if not _no_gpu():
        pytest.skip("GPU present")
    from circl_amd import hostapi as api
    s = api.HpkeSuite(0x20, 1, 3)
    z = np.zeros((2, 32), np.uint8)
    ctx = np.zeros((2, 80), np.uint8)
    for f in (lambda: s.setup_sender(0, z, z), lambda: s.setup_receiver(0, z, z), lambda: s.seal(ctx, [b"a", b""]), lambda: s.open(ctx, [bytes(16), bytes(17)]),
              lambda: s.export(ctx, None, 32), lambda: s.seal_single(0, z, z, [b"a", b"bc"]), lambda: s.open_single(0, z, z, [bytes(16), bytes(20)]),
              lambda: s.export_single(0, z, z, None, 5), lambda: s.export_single_receiver(0, z, z, [b"x", b"y"], 5)):
        with pytest.raises(nat.CirclHipError) as e:
            f()
        assert e.value.code == nat.ENODEV
    with pytest.raises(ValueError):
        api.HpkeSuite(0x10, 1, 3)
    with pytest.raises(ValueError):
        api.HpkeSuite(0x20, 2, 3)
    with pytest.raises(ValueError):
        api.HpkeSuite(0x20, 1, 1)
