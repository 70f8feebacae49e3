"""CPU-side checks of the NIST-curve DLEQ / POPRF entry points of the C ABI, in both forms and on both curves: the argument contract,
which is checked before any device is looked for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud
failure of every well-formed call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from circl_amd import _native as nat
from circl_amd import build as cbuild

KEEP = np.zeros(8192, np.uint8)
P = KEEP.ctypes.data_as(C.c_void_p)
OFF = np.array([0, 1, 1, 1], np.uint64)
O = OFF.ctypes.data_as(C.c_void_p)
DOWN = np.array([0, 2, 1, 3], np.uint64)
LATE = np.array([1, 2, 3, 4], np.uint64)

ENTRY = {   # name -> its arguments after the curve and before the counts, in order
    "nistp_dleq_prove": ["k", "k_stride", "kA", "kA_stride", "B", "kB", "off", "r", "dst", "dst_len", "flags", "proofs", "ok"],
    "nistp_dleq_verify": ["kA", "kA_stride", "B", "kB", "off", "proofs", "dst", "dst_len", "flags", "ok"],
    "oprf_nistp_poprf_tweak": ["sk", "sk_stride", "pkS", "pk_stride", "info", "off", "t", "t_inv", "tweaked", "ok"],
    "oprf_nistp_poprf_finalize": ["blob", "off", "info", "off", "blinds", "evaluated", "out", "ok"],
    "oprf_nistp_poprf_full_evaluate": ["sk", "sk_stride", "blob", "off", "info", "off", "out", "ok"],
}
NS, NE = {256: 32, 384: 48}, {256: 33, 384: 49}
DLEQ = ("nistp_dleq_prove", "nistp_dleq_verify")
CURVES = (256, 384)
FORMS = [(e, s, c) for e in ENTRY for s in ("", "_dev") for c in CURVES]
DLEQ_FORMS = [f for f in FORMS if f[0] in DLEQ]


def scalars(curve):
    return dict(k_stride=NS[curve], kA_stride=NE[curve], sk_stride=NS[curve], pk_stride=NE[curve], dst_len=27, flags=0)


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def call(lib, entry, suffix, curve, n=1, **over):
    """the entry point with well-formed arguments, except for `over`"""
    over = dict(over)
    if entry == "oprf_nistp_poprf_tweak" and "pkS" not in over and "sk" not in over:
        over["pkS"] = None                                      # the server's side
    sc = scalars(curve if curve in NS else 256)
    args = [over[a] if a in over else sc[a] if a in sc else O if a == "off" else P for a in ENTRY[entry]]
    fn = getattr(lib, "circl_hip_" + entry + suffix)
    if entry in DLEQ and suffix:
        n_elems = over.get("n_elems", 1)
        return fn(curve, *args, n, n_elems, over.get("ws", P), over.get("ws_bytes", lib.circl_hip_nistp_dleq_workspace_size(curve, n, n_elems)), None)
    return fn(curve, *args, n, None if suffix else 0)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_every_symbol_is_declared_and_listed():
    with open(os.path.join(cbuild.ROOT, "include", "circl_hip.h")) as f:
        h = f.read()
    for e in ENTRY:
        for s in ("", "_dev"):
            assert "circl_hip_" + e + s in nat.SYMBOLS
            assert re.search(r"\bint circl_hip_%s%s\(int curve, " % (e, s), h)
    assert "circl_hip_nistp_dleq_workspace_size" in nat.SYMBOLS and "size_t circl_hip_nistp_dleq_workspace_size(int curve, " in h


def test_the_library_exports_every_symbol(L):
    for e in ENTRY:
        for s in ("", "_dev"):
            assert getattr(L, "circl_hip_" + e + s) is not None
    assert L.circl_hip_nistp_dleq_workspace_size(256, 1, 1) > 0


@pytest.mark.parametrize("entry,suffix,curve", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix, curve):
    assert call(L, entry, suffix, curve, n=0) == nat.OK
    if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
        assert call(L, entry, suffix, curve) == nat.ENODEV
        assert call(L, entry, suffix, curve, 3) == nat.ENODEV
        if entry == "oprf_nistp_poprf_tweak":
            assert call(L, entry, suffix, curve, sk=None, t=None, t_inv=None) == nat.ENODEV        # the client's side


@pytest.mark.parametrize("entry,suffix,curve", FORMS)
def test_curves(L, entry, suffix, curve):
    for bad in (0, 1, 255, 257, 521, 25519, -256):
        for n in (0, 1):
            assert call(L, entry, suffix, bad, n, **scalars(curve)) == nat.EPARAM, bad
    assert L.circl_hip_nistp_dleq_workspace_size(521, 1, 1) == 0


@pytest.mark.parametrize("entry,suffix,curve", FORMS)
def test_strides(L, entry, suffix, curve):
    other = 384 + 256 - curve
    for name in [a for a in ENTRY[entry] if a.endswith("_stride")]:
        right = scalars(curve)[name]
        wrong = {1, 4, 31, 32, 33, 48, 49, 64, 96, scalars(other)[name]} - {right}
        for n in (0, 1):
            for stride in sorted(wrong):
                assert call(L, entry, suffix, curve, n, **{name: stride}) == nat.EPARAM, (name, stride)
        for stride in (0, right):
            assert call(L, entry, suffix, curve, 0, **{name: stride}) == nat.OK
            if _no_gpu():
                assert call(L, entry, suffix, curve, 1, **{name: stride}) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix,curve", DLEQ_FORMS)
def test_tags_and_flags(L, entry, suffix, curve):
    for n in (0, 1):
        for dl in (243, 255, 1000):
            assert call(L, entry, suffix, curve, n, dst_len=dl) == nat.EPARAM, dl
        assert call(L, entry, suffix, curve, n, dst=None) == nat.EPARAM
        for flags in (2, 3, 0x80000000):
            assert call(L, entry, suffix, curve, n, flags=flags) == nat.EPARAM
    for dl in (0, 1, 242):
        assert call(L, entry, suffix, curve, 0, dst_len=dl) == nat.OK
    assert call(L, entry, suffix, curve, 0, dst=None, dst_len=0) == nat.OK
    assert call(L, entry, suffix, curve, 0, flags=1) == nat.OK
    if _no_gpu():
        assert call(L, entry, suffix, curve, dst_len=242, flags=1) == nat.ENODEV
        assert call(L, entry, suffix, curve, dst=None, dst_len=0) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix,curve", FORMS)
def test_null_pointers(L, entry, suffix, curve):
    required = {"nistp_dleq_prove": ("k", "kA", "B", "kB", "off", "r", "proofs"), "nistp_dleq_verify": ("kA", "B", "kB", "off", "proofs", "ok"),
                "oprf_nistp_poprf_tweak": ("t", "t_inv", "tweaked"), "oprf_nistp_poprf_finalize": ("blinds", "evaluated", "out"),
                "oprf_nistp_poprf_full_evaluate": ("sk", "out")}[entry]
    for a in required:
        assert call(L, entry, suffix, curve, **{a: None}) == nat.EPARAM, a
    if entry == "oprf_nistp_poprf_tweak":
        assert call(L, entry, suffix, curve, pkS=P) == nat.EPARAM                       # both sides at once
        assert call(L, entry, suffix, curve, sk=None, pkS=None) == nat.EPARAM           # neither
        assert call(L, entry, suffix, curve, sk=None, tweaked=None) == nat.EPARAM       # the client's one output
    if entry.startswith("oprf_nistp_poprf"):
        assert call(L, entry, suffix, curve, off=None) == nat.EPARAM                    # a blob without offsets
    if _no_gpu() and entry != "nistp_dleq_verify":
        assert call(L, entry, suffix, curve, ok=None) == nat.ENODEV                     # ok may be NULL (not the verdict of verify)
    if _no_gpu() and entry.startswith("oprf_nistp_poprf"):
        assert call(L, entry, suffix, curve, info=None) == nat.ENODEV                   # no blob: every item's info is empty


@pytest.mark.parametrize("entry", DLEQ)
@pytest.mark.parametrize("curve", CURVES)
def test_request_offsets_of_the_host_form(L, entry, curve):
    assert call(L, entry, "", curve, 3, off=DOWN.ctypes.data_as(C.c_void_p)) == nat.EPARAM
    assert call(L, entry, "", curve, 3, off=LATE.ctypes.data_as(C.c_void_p)) == nat.EPARAM
    assert call(L, entry, "", curve, 0, off=DOWN.ctypes.data_as(C.c_void_p)) == nat.OK


@pytest.mark.parametrize("curve", CURVES)
def test_workspace_and_alignment(L, curve):
    ws = lambda r, e: L.circl_hip_nistp_dleq_workspace_size(curve, r, e)
    sizes = [(0, 0), (1, 0), (1, 1), (1, 64), (1, 65), (2, 65), (300, 750), (1, 65535), (1 << 14, 1 << 20), (1 << 20, 1 << 20)]
    for (r0, e0), (r1, e1) in zip(sizes, sizes[1:]):
        assert ws(r0, e0) <= ws(r1, e1)
    slot = 2 * 3 * (NS[curve] // 4) * 4                                                # two points of 3 N words
    assert ws(1 << 14, 1 << 20) <= (slot // 64 + 1) * (1 << 20) + (slot + 4) * (1 << 14) + 512
    odd = C.c_void_p(KEEP.ctypes.data + 1)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    for entry in DLEQ:
        assert call(L, entry, "_dev", curve, 3, ws_bytes=ws(3, 1) - 1) == nat.EWORKSPACE
        assert call(L, entry, "_dev", curve, 1, n_elems=65, ws_bytes=ws(1, 64)) == nat.EWORKSPACE
        assert call(L, entry, "_dev", curve, ws=None) == nat.EWORKSPACE
        assert call(L, entry, "_dev", curve, ws=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", curve, proofs=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", curve, off=odd4) == nat.EWORKSPACE
        if _no_gpu():                                                                  # element rows may lie anywhere
            assert call(L, entry, "_dev", curve, B=odd, kB=odd, kA=odd) == nat.ENODEV
    assert call(L, "nistp_dleq_prove", "_dev", curve, k=odd) == nat.EWORKSPACE
    assert call(L, "nistp_dleq_prove", "_dev", curve, r=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_poprf_finalize", "_dev", curve, blinds=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_poprf_finalize", "_dev", curve, out=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_poprf_full_evaluate", "_dev", curve, off=odd4) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_poprf_tweak", "_dev", curve, t_inv=odd) == nat.EWORKSPACE
    assert call(L, "oprf_nistp_poprf_tweak", "_dev", curve, t=odd) == nat.EWORKSPACE
    if _no_gpu():
        assert call(L, "oprf_nistp_poprf_finalize", "_dev", curve, evaluated=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_poprf_tweak", "_dev", curve, tweaked=odd) == nat.ENODEV
        assert call(L, "oprf_nistp_poprf_tweak", "_dev", curve, sk=None, pkS=odd, tweaked=odd) == nat.ENODEV


def test_the_base_mode_full_evaluate_still_refuses_mode_2(L):
    for curve in CURVES:
        assert L.circl_hip_oprf_nistp_full_evaluate(curve, 2, P, NS[curve], P, O, P, P, 1, 0) == nat.EPARAM
