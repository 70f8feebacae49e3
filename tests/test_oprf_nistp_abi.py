"""CPU-side checks of the P-256 / P-384 group and OPRF entry points of the C ABI: the argument contract, which is checked before any device
is looked for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure of every well-formed call."""
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
    "nistp_hash_to_group": ["curve", "blob", "off", "dst", "dst_len", "flags", "out"],
    "nistp_hash_to_scalar": ["curve", "blob", "off", "dst", "dst_len", "out"],
    "nistp_scalar_mult": ["curve", "scalars", "stride", "elems", "flags", "out", "ok"],
    "oprf_nistp_derive_keypair": ["curve", "mode", "seeds", "blob", "off", "sk", "pk", "ok"],
    "oprf_nistp_blind": ["curve", "mode", "blob", "off", "blinds", "out", "ok"],
    "oprf_nistp_evaluate": ["curve", "sk", "stride", "blinded", "out", "ok"],
    "oprf_nistp_finalize": ["curve", "blob", "off", "blinds", "evaluated", "out", "ok"],
    "oprf_nistp_full_evaluate": ["curve", "mode", "sk", "stride", "blob", "off", "out", "ok"],
}
CURVES = (256, 384)
CASES = [(e, s, c) for e in ENTRY for s in ("", "_dev") for c in CURVES]
OUTPUTS = ("out", "sk", "pk")                                             # required; ok may be NULL
REQUIRED_INPUTS = ("scalars", "seeds", "blinds", "blinded", "evaluated", "dst")


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def call(lib, entry, suffix, curve, n=1, **over):
    """the entry point with well-formed arguments for the curve, except for `over`"""
    scalars = dict(curve=curve, dst_len=40, stride=curve // 8, flags=0, mode=0)
    args = []
    for a in ENTRY[entry]:
        if a in over:
            v = over[a]
        elif a in scalars:
            v = scalars[a]
        else:
            v = O if a == "off" else P
        args.append(v)
    return getattr(lib, "circl_hip_" + entry + suffix)(*args, n, None if suffix else 0)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_every_symbol_is_declared_and_listed(L):
    for e in ENTRY:
        for s in ("", "_dev"):
            assert "circl_hip_" + e + s in nat.SYMBOLS and hasattr(L, "circl_hip_" + e + s)


@pytest.mark.parametrize("entry,suffix,curve", CASES)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix, curve):
    assert call(L, entry, suffix, curve, n=0) == nat.OK
    if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
        assert call(L, entry, suffix, curve) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", [(e, s) for e in ENTRY for s in ("", "_dev")])
def test_curves(L, entry, suffix):
    for n in (0, 1):
        for curve in (0, 1, 255, 257, 383, 521, 25519, -256):
            assert call(L, entry, suffix, curve, n, stride=32) == nat.EPARAM, curve


@pytest.mark.parametrize("entry,suffix,curve", [x for x in CASES if "mode" in ENTRY[x[0]]])
def test_modes(L, entry, suffix, curve):
    top = 1 if entry == "oprf_nistp_full_evaluate" else 2        # FullEvaluate of mode 2 needs the info tweak
    for n in (0, 1):
        for mode in (top + 1, 3, 4, -1, 255):
            assert call(L, entry, suffix, curve, n, mode=mode) == nat.EPARAM, mode
    for mode in range(top + 1):
        assert call(L, entry, suffix, curve, 0, mode=mode) == nat.OK


@pytest.mark.parametrize("suffix", ["", "_dev"])
@pytest.mark.parametrize("curve", CURVES)
def test_dst_lengths(L, suffix, curve):
    for entry in ("nistp_hash_to_group", "nistp_hash_to_scalar"):
        for n in (0, 1):
            for dl in (0, 256, 1000):
                assert call(L, entry, suffix, curve, n, dst_len=dl) == nat.EPARAM, dl
            assert call(L, entry, suffix, curve, n, dst=None) == nat.EPARAM
        for dl in (1, 255):
            assert call(L, entry, suffix, curve, 0, dst_len=dl) == nat.OK


@pytest.mark.parametrize("suffix", ["", "_dev"])
@pytest.mark.parametrize("curve", CURVES)
def test_strides_and_flags(L, suffix, curve):
    other = 48 if curve == 256 else 32                           # the other curve's row is not this one's
    for entry in ("nistp_scalar_mult", "oprf_nistp_evaluate", "oprf_nistp_full_evaluate"):
        for n in (0, 1):
            for stride in (1, 4, 31, 33, 49, 64, 96, other):
                assert call(L, entry, suffix, curve, n, stride=stride) == nat.EPARAM, (entry, stride)
        for stride in (0, curve // 8):
            assert call(L, entry, suffix, curve, 0, stride=stride) == nat.OK
    for entry in ("nistp_scalar_mult", "nistp_hash_to_group"):
        for n in (0, 1):
            for flags in (2, 3, 0x80000000):
                assert call(L, entry, suffix, curve, n, flags=flags) == nat.EPARAM
        assert call(L, entry, suffix, curve, 0, flags=1) == nat.OK


@pytest.mark.parametrize("entry,suffix,curve", CASES)
def test_null_pointers(L, entry, suffix, curve):
    names = ENTRY[entry]
    for a in names:
        if a in OUTPUTS or a in REQUIRED_INPUTS or a == "sk":
            assert call(L, entry, suffix, curve, **{a: None}) == nat.EPARAM, a
            assert call(L, entry, suffix, curve, 0, **{a: None}) in (nat.OK, nat.EPARAM)
    if "blob" in names:
        assert call(L, entry, suffix, curve, off=None) == nat.EPARAM          # a blob without offsets
        if _no_gpu():
            assert call(L, entry, suffix, curve, blob=None, off=None) == nat.ENODEV      # no blob: every item's input is empty
            assert call(L, entry, suffix, curve, blob=None) == nat.ENODEV
    if "ok" in names and _no_gpu():
        assert call(L, entry, suffix, curve, ok=None) == nat.ENODEV          # ok may be NULL
    if entry == "nistp_scalar_mult" and _no_gpu():
        assert call(L, entry, suffix, curve, elems=None) == nat.ENODEV       # the generator


@pytest.mark.parametrize("curve", CURVES)
def test_misaligned_device_pointers(L, curve):
    """rows of words (scalars, seeds, scalar and hash outputs) want 4-byte alignment, offsets 8; element rows are packed and may lie anywhere"""
    odd = C.c_void_p(KEEP.ctypes.data + 1)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    assert call(L, "nistp_hash_to_scalar", "_dev", curve, out=odd) == nat.EWORKSPACE
    assert call(L, "nistp_hash_to_group", "_dev", curve, off=odd4) == nat.EWORKSPACE
    assert call(L, "nistp_scalar_mult", "_dev", curve, scalars=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_derive_keypair", "_dev", curve, seeds=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_derive_keypair", "_dev", curve, sk=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_blind", "_dev", curve, blinds=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_evaluate", "_dev", curve, sk=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_finalize", "_dev", curve, out=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_finalize", "_dev", curve, off=odd4) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_full_evaluate", "_dev", curve, out=odd) == nat.EWORKSPACE
    if _no_gpu():       # packed element rows: an odd address passes the contract
        assert call(L, "nistp_hash_to_group", "_dev", curve, out=odd) == nat.ENODEV
        assert call(L, "nistp_scalar_mult", "_dev", curve, elems=odd, out=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_derive_keypair", "_dev", curve, pk=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_blind", "_dev", curve, out=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_evaluate", "_dev", curve, blinded=odd, out=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_finalize", "_dev", curve, evaluated=odd) == nat.ENODEV


@pytest.mark.parametrize("curve", CURVES)
def test_no_gpu_means_loud_failure(curve):
    from circl_amd import hostapi as api
    g = api.NistpOprf(curve)
    with pytest.raises(nat.CirclHipError) as e:
        g.full_evaluate(2, bytes(g.Ns), [b"x"])
    assert e.value.code == nat.EPARAM
    with pytest.raises(nat.CirclHipError) as e:
        g.hash_to_group([b"x"], b"")
    assert e.value.code == nat.EPARAM
    with pytest.raises(ValueError):
        api.NistpOprf(521)
    if not _no_gpu():
        return
    z, e2 = np.zeros((2, g.Ns), np.uint8), np.zeros((2, g.Ne), np.uint8)
    for f in (lambda: g.hash_to_group([b"a", b""], b"dst"), lambda: g.hash_to_group([b"a", b""], b"dst", nonuniform=True),
              lambda: g.hash_to_scalar([b"a", b""], b"dst"), lambda: g.scalar_mult(z), lambda: g.scalar_mult(bytes(g.Ns), e2, invert=True),
              lambda: g.derive_keypair(0, np.zeros((2, 32), np.uint8), [b"info", b""]), lambda: g.blind(1, [b"x", b"y"], z),
              lambda: g.evaluate(bytes(g.Ns), e2), lambda: g.evaluate(z, e2), lambda: g.finalize([b"x", b"y"], z, e2),
              lambda: g.full_evaluate(0, bytes(g.Ns), [b"x", b"y"])):
        with pytest.raises(nat.CirclHipError) as e:
            f()
        assert e.value.code == nat.ENODEV
