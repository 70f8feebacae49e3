"""CPU-side checks of the ristretto255 / OPRF entry points of the C ABI: the argument contract, which is checked before any device is
looked for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure of every well-formed call."""
import ctypes as C

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

KEEP = np.zeros(4096, np.uint8)
P = KEEP.ctypes.data_as(C.c_void_p)
OFF = np.zeros(8, np.uint64)
O = OFF.ctypes.data_as(C.c_void_p)

ENTRY = {   # name -> its arguments before n, in order
    "ristretto255_hash_to_group": ["blob", "off", "dst", "dst_len", "out"],
    "ristretto255_hash_to_scalar": ["blob", "off", "dst", "dst_len", "out"],
    "ristretto255_scalar_mult": ["scalars", "stride", "elems", "flags", "out", "ok"],
    "oprf_derive_keypair": ["mode", "seeds", "blob", "off", "sk", "pk", "ok"],
    "oprf_blind": ["mode", "blob", "off", "blinds", "out", "ok"],
    "oprf_evaluate": ["sk", "stride", "blinded", "out", "ok"],
    "oprf_finalize": ["blob", "off", "blinds", "evaluated", "out", "ok"],
    "oprf_full_evaluate": ["mode", "sk", "stride", "blob", "off", "out", "ok"],
}
SCALARS = dict(dst_len=40, stride=32, flags=0, mode=0)
FORMS = [(e, s) for e in ENTRY for s in ("", "_dev")]
OUTPUTS = ("out", "sk", "pk")                                             # required; ok may be NULL
REQUIRED_INPUTS = ("scalars", "seeds", "blinds", "blinded", "evaluated", "dst")


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def call(lib, entry, suffix, n=1, **over):
    """the entry point with well-formed arguments, except for `over`"""
    args = []
    for a in ENTRY[entry]:
        if a in over:
            v = over[a]
        elif a in SCALARS:
            v = SCALARS[a]
        else:
            v = O if a == "off" else P
        args.append(v)
    return getattr(lib, "circl_hip_" + entry + suffix)(*args, n, None if suffix else 0)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_every_symbol_is_declared_and_listed():
    for e in ENTRY:
        for s in ("", "_dev"):
            assert "circl_hip_" + e + s in nat.SYMBOLS


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    assert call(L, entry, suffix, n=0) == nat.OK
    if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
        assert call(L, entry, suffix) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", [(e, s) for e, s in FORMS if "mode" in ENTRY[e]])
def test_modes(L, entry, suffix):
    top = 1 if entry == "oprf_full_evaluate" else 2        # FullEvaluate of mode 2 needs the info tweak
    for n in (0, 1):
        for mode in (top + 1, 3, 4, -1, 255):
            assert call(L, entry, suffix, n, mode=mode) == nat.EPARAM, mode
    for mode in range(top + 1):
        assert call(L, entry, suffix, 0, mode=mode) == nat.OK


@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_dst_lengths(L, suffix):
    for entry in ("ristretto255_hash_to_group", "ristretto255_hash_to_scalar"):
        for n in (0, 1):
            for dl in (0, 256, 1000):
                assert call(L, entry, suffix, n, dst_len=dl) == nat.EPARAM, dl
            assert call(L, entry, suffix, n, dst=None) == nat.EPARAM
        for dl in (1, 255):
            assert call(L, entry, suffix, 0, dst_len=dl) == nat.OK


@pytest.mark.parametrize("suffix", ["", "_dev"])
def test_strides_and_flags(L, suffix):
    for entry in ("ristretto255_scalar_mult", "oprf_evaluate", "oprf_full_evaluate"):
        for n in (0, 1):
            for stride in (1, 4, 31, 33, 64):
                assert call(L, entry, suffix, n, stride=stride) == nat.EPARAM, (entry, stride)
        for stride in (0, 32):
            assert call(L, entry, suffix, 0, stride=stride) == nat.OK
    for n in (0, 1):
        for flags in (2, 3, 0x80000000):
            assert call(L, "ristretto255_scalar_mult", suffix, n, flags=flags) == nat.EPARAM
    assert call(L, "ristretto255_scalar_mult", suffix, 0, flags=1) == nat.OK


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_null_pointers(L, entry, suffix):
    names = ENTRY[entry]
    for a in names:
        if a in OUTPUTS or a in REQUIRED_INPUTS or a == "sk":
            assert call(L, entry, suffix, **{a: None}) == nat.EPARAM, a
            assert call(L, entry, suffix, 0, **{a: None}) in (nat.OK, nat.EPARAM)
    if "blob" in names:
        assert call(L, entry, suffix, off=None) == nat.EPARAM                # a blob without offsets
        ok_rc = (nat.ENODEV,) if _no_gpu() else ()
        if ok_rc:
            assert call(L, entry, suffix, blob=None, off=None) in ok_rc      # no blob: every item's input is empty
            assert call(L, entry, suffix, blob=None) in ok_rc
    if "ok" in names and _no_gpu():
        assert call(L, entry, suffix, ok=None) == nat.ENODEV                 # ok may be NULL
    if entry == "ristretto255_scalar_mult" and _no_gpu():
        assert call(L, entry, suffix, elems=None) == nat.ENODEV              # the generator


def test_misaligned_device_pointers(L):
    odd = C.c_void_p(KEEP.ctypes.data + 1)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    assert call(L, "ristretto255_hash_to_group", "_dev", out=odd) == nat.EWORKSPACE
    assert call(L, "ristretto255_hash_to_scalar", "_dev", off=odd4) == nat.EWORKSPACE
    assert call(L, "ristretto255_scalar_mult", "_dev", scalars=odd) == nat.EWORKSPACE
    assert call(L, "oprf_derive_keypair", "_dev", pk=odd) == nat.EWORKSPACE
    assert call(L, "oprf_blind", "_dev", blinds=odd) == nat.EWORKSPACE
    assert call(L, "oprf_evaluate", "_dev", blinded=odd) == nat.EWORKSPACE
    assert call(L, "oprf_finalize", "_dev", off=odd4) == nat.EWORKSPACE
    assert call(L, "oprf_full_evaluate", "_dev", sk=odd) == nat.EWORKSPACE
    # element rows are read and written as words in this group
    assert call(L, "ristretto255_scalar_mult", "_dev", elems=odd) == nat.EWORKSPACE
    assert call(L, "oprf_blind", "_dev", out=odd) == nat.EWORKSPACE
    assert call(L, "oprf_finalize", "_dev", evaluated=odd) == nat.EWORKSPACE


def test_no_gpu_means_loud_failure():
    if not _no_gpu():
        pytest.skip("GPU present")
    from circl_amd import hostapi as api
    z = np.zeros((2, 32), np.uint8)
    for f in (lambda: api.ristretto255_hash_to_group([b"a", b""], b"dst"), lambda: api.ristretto255_hash_to_scalar([b"a", b""], b"dst"),
              lambda: api.ristretto255_scalar_mult(z), lambda: api.ristretto255_scalar_mult(bytes(32), z, invert=True),
              lambda: api.oprf_derive_keypair(0, z, [b"info", b""]), lambda: api.oprf_blind(1, [b"x", b"y"], z),
              lambda: api.oprf_evaluate(bytes(32), z), lambda: api.oprf_evaluate(z, z), lambda: api.oprf_finalize([b"x", b"y"], z, z),
              lambda: api.oprf_full_evaluate(0, bytes(32), [b"x", b"y"])):
        with pytest.raises(nat.CirclHipError) as e:
            f()
        assert e.value.code == nat.ENODEV
    with pytest.raises(nat.CirclHipError) as e:
        api.oprf_full_evaluate(2, bytes(32), [b"x"])
    assert e.value.code == nat.EPARAM
    with pytest.raises(nat.CirclHipError) as e:
        api.ristretto255_hash_to_group([b"x"], b"")
    assert e.value.code == nat.EPARAM
