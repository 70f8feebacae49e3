"""CPU-side checks of the DLEQ / POPRF entry points of the C ABI: the argument contract, which is checked before any device is looked
for (so a breach is CIRCL_HIP_EPARAM with or without a GPU) and, without a GPU, the loud failure of every well-formed call."""
import ctypes as C

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

ENTRY = {   # name -> its arguments before the counts, in order
    "dleq_prove": ["k", "k_stride", "kA", "kA_stride", "B", "kB", "off", "r", "dst", "dst_len", "flags", "proofs", "ok"],
    "dleq_verify": ["kA", "kA_stride", "B", "kB", "off", "proofs", "dst", "dst_len", "flags", "ok"],
    "oprf_poprf_tweak": ["sk", "sk_stride", "pkS", "pk_stride", "info", "off", "t", "t_inv", "tweaked", "ok"],
    "oprf_poprf_finalize": ["blob", "off", "info", "off", "blinds", "evaluated", "out", "ok"],
    "oprf_poprf_full_evaluate": ["sk", "sk_stride", "blob", "off", "info", "off", "out", "ok"],
}
SCALARS = dict(k_stride=32, kA_stride=32, sk_stride=32, pk_stride=32, dst_len=27, flags=0)
DLEQ = ("dleq_prove", "dleq_verify")
FORMS = [(e, s) for e in ENTRY for s in ("", "_dev")]


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def call(lib, entry, suffix, n=1, **over):
    """the entry point with well-formed arguments, except for `over`"""
    over = dict(over)
    if entry == "oprf_poprf_tweak" and "pkS" not in over and "sk" not in over:
        over["pkS"] = None                                      # the server's side
    args = [over[a] if a in over else SCALARS[a] if a in SCALARS else O if a == "off" else P for a in ENTRY[entry]]
    fn = getattr(lib, "circl_hip_" + entry + suffix)
    if entry in DLEQ and suffix:
        n_elems = over.get("n_elems", 1)
        return fn(*args, n, n_elems, over.get("ws", P), over.get("ws_bytes", lib.circl_hip_dleq_workspace_size(n, n_elems)), None)
    return fn(*args, n, None if suffix else 0)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_every_symbol_is_declared_and_listed():
    for e in ENTRY:
        for s in ("", "_dev"):
            assert "circl_hip_" + e + s in nat.SYMBOLS
    assert "circl_hip_dleq_workspace_size" in nat.SYMBOLS


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    assert call(L, entry, suffix, n=0) == nat.OK
    if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
        assert call(L, entry, suffix) == nat.ENODEV
        assert call(L, entry, suffix, 3) == nat.ENODEV
        if entry == "oprf_poprf_tweak":
            assert call(L, entry, suffix, sk=None, t=None, t_inv=None) == nat.ENODEV        # the client's side


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_strides(L, entry, suffix):
    for name in [a for a in ENTRY[entry] if a.endswith("_stride")]:
        for n in (0, 1):
            for stride in (1, 4, 31, 33, 64):
                assert call(L, entry, suffix, n, **{name: stride}) == nat.EPARAM, (name, stride)
        for stride in (0, 32):
            assert call(L, entry, suffix, 0, **{name: stride}) == nat.OK


@pytest.mark.parametrize("entry,suffix", [(e, s) for e in DLEQ for s in ("", "_dev")])
def test_tags_and_flags(L, entry, suffix):
    for n in (0, 1):
        for dl in (243, 255, 1000):
            assert call(L, entry, suffix, n, dst_len=dl) == nat.EPARAM, dl
        assert call(L, entry, suffix, n, dst=None) == nat.EPARAM
        for flags in (2, 3, 0x80000000):
            assert call(L, entry, suffix, n, flags=flags) == nat.EPARAM
    for dl in (0, 1, 242):
        assert call(L, entry, suffix, 0, dst_len=dl) == nat.OK
    assert call(L, entry, suffix, 0, dst=None, dst_len=0) == nat.OK
    assert call(L, entry, suffix, 0, flags=1) == nat.OK
    if _no_gpu():
        assert call(L, entry, suffix, dst_len=242, flags=1) == nat.ENODEV
        assert call(L, entry, suffix, dst=None, dst_len=0) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_null_pointers(L, entry, suffix):
    required = {"dleq_prove": ("k", "kA", "B", "kB", "off", "r", "proofs"), "dleq_verify": ("kA", "B", "kB", "off", "proofs", "ok"),
                "oprf_poprf_tweak": ("t", "t_inv", "tweaked"), "oprf_poprf_finalize": ("blinds", "evaluated", "out"),
                "oprf_poprf_full_evaluate": ("sk", "out")}[entry]
    for a in required:
        assert call(L, entry, suffix, **{a: None}) == nat.EPARAM, a
    if entry == "oprf_poprf_tweak":
        assert call(L, entry, suffix, pkS=P) == nat.EPARAM                       # both sides at once
        assert call(L, entry, suffix, sk=None, pkS=None) == nat.EPARAM           # neither
        assert call(L, entry, suffix, sk=None, tweaked=None) == nat.EPARAM       # the client's one output
    if entry.startswith("oprf_poprf"):
        assert call(L, entry, suffix, off=None) == nat.EPARAM                    # a blob without offsets
    if _no_gpu() and entry != "dleq_verify":
        assert call(L, entry, suffix, ok=None) == nat.ENODEV                     # ok may be NULL (not the verdict of verify)
    if _no_gpu() and entry.startswith("oprf_poprf"):
        assert call(L, entry, suffix, info=None) == nat.ENODEV                   # no blob: every item's info is empty


@pytest.mark.parametrize("entry", DLEQ)
def test_request_offsets_of_the_host_form(L, entry):
    assert call(L, entry, "", 3, off=DOWN.ctypes.data_as(C.c_void_p)) == nat.EPARAM
    assert call(L, entry, "", 3, off=LATE.ctypes.data_as(C.c_void_p)) == nat.EPARAM
    assert call(L, entry, "", 0, off=DOWN.ctypes.data_as(C.c_void_p)) == nat.OK


def test_workspace(L):
    ws = L.circl_hip_dleq_workspace_size
    sizes = [(0, 0), (1, 0), (1, 1), (1, 64), (1, 65), (2, 65), (300, 750), (1, 65535), (1 << 14, 1 << 20), (1 << 20, 1 << 20)]
    for (r0, e0), (r1, e1) in zip(sizes, sizes[1:]):
        assert ws(r0, e0) <= ws(r1, e1)
    assert ws(1 << 14, 1 << 20) <= 5 * (1 << 20) + 324 * (1 << 14) + 512         # about 5 bytes per element and 320 per request
    odd = C.c_void_p(KEEP.ctypes.data + 1)
    odd4 = C.c_void_p(OFF.ctypes.data + 4)
    for entry in DLEQ:
        assert call(L, entry, "_dev", 3, ws_bytes=ws(3, 1) - 1) == nat.EWORKSPACE
        assert call(L, entry, "_dev", 1, n_elems=65, ws_bytes=ws(1, 64)) == nat.EWORKSPACE
        assert call(L, entry, "_dev", ws=None) == nat.EWORKSPACE
        assert call(L, entry, "_dev", ws=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", B=odd) == nat.EWORKSPACE
        assert call(L, entry, "_dev", off=odd4) == nat.EWORKSPACE
    assert call(L, "oprf_poprf_finalize", "_dev", blinds=odd) == nat.EWORKSPACE
    assert call(L, "oprf_poprf_full_evaluate", "_dev", off=odd4) == nat.EWORKSPACE
    assert call(L, "oprf_poprf_tweak", "_dev", t_inv=odd) == nat.EWORKSPACE


def test_the_base_mode_full_evaluate_still_refuses_mode_2(L):
    assert L.circl_hip_oprf_full_evaluate(2, P, 32, P, O, P, P, 1, 0) == nat.EPARAM
