"""CPU-side checks of the Ascon device source: the item functions of ascon_kernels.h compiled for the host
(tests/hostsim/ascon_hostsim.hip) on every vector of the fixture and on a ragged batch with distinct keys against the checker
tests/ascon.py, and the same source as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ascon
from test_oracle_ascon import flip, vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "ascon_hostsim.hip")
vp, sz = C.c_void_p, C.c_size_t
NAMES = sorted(ascon.MODES)


class Args(C.Structure):  # ascon_kernels.h Args
    _fields_ = [("key", vp), ("key_stride_words", sz), ("nonce", vp), ("in_", vp), ("aad", vp), ("pt_off", vp), ("aad_off", vp), ("out", vp), ("ok", vp),
                ("n", sz)]


def _stale(out):
    from circl_amd import build
    deps = [SRC] + [os.path.join(build.CSRC, h) for h in ("ascon_dev.h", "ascon_kernels.h", "keccak_dev.h")]
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


def _hipcc(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def hs():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libascon_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_ascon_call.argtypes = [C.c_int, C.c_int, vp]
    lib.hs_ascon_perm.argtypes = [C.c_int, vp]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _rows(rows, stride):
    """a fresh word-aligned array holding the rows `stride` bytes apart"""
    a = np.zeros(max(1, len(rows) * stride // 4), np.uint32)
    b = a.view(np.uint8)
    for j, r in enumerate(rows):
        b[j * stride:j * stride + len(r)] = np.frombuffer(bytes(r), np.uint8)
    return a


def _blob(items, lead=0, base=0):
    """(array, view whose address is `base` past a word boundary, offsets starting at `lead`)"""
    off = np.array([lead + sum(len(x) for x in items[:j]) for j in range(len(items) + 1)], np.uint64)
    keep = np.zeros((int(off[-1]) + base) // 4 + 2, np.uint32)
    view = keep.view(np.uint8)[base:base + int(off[-1])]
    view[lead:] = np.frombuffer(b"".join(bytes(x) for x in items), np.uint8)
    return keep, view, off


def sim(hs, mode, seal, keys, nonces, texts, aads=None, key_stride=None, lead=0, base=0, guard=16):
    """One call through the host instantiation.  keys: one key (shared) or a list.  texts: plaintexts (seal) or ciphertexts (open).
    Returns the ciphertexts, or (plaintexts, ok).  The output blob has `guard` sentinel bytes on each side."""
    n, ks = len(texts), ascon.key_size(mode)
    shared = isinstance(keys, bytes)
    stride = 0 if shared else (key_stride or ks)
    k, nn = _rows([keys] if shared else keys, stride or ks), _rows(nonces, 16)
    pts = texts if seal else [t[:-16] for t in texts]
    _, _, off = _blob(pts, lead)
    pad_in, pad_out = (0, 16) if seal else (16, 0)
    # the input blob: item i at off[i] + pad_in * i
    in_keep = np.zeros((int(off[-1]) + pad_in * n + base) // 4 + 2, np.uint32)
    in_view = in_keep.view(np.uint8)[base:]
    for j, t in enumerate(texts):
        at = int(off[j]) + pad_in * j
        in_view[at:at + len(t)] = np.frombuffer(bytes(t), np.uint8)
    out_len = int(off[-1]) + pad_out * n
    out_keep = np.full((out_len + base + 2 * guard) // 4 + 2, 0xA5A5A5A5, np.uint32)
    out_view = out_keep.view(np.uint8)[base + guard:base + guard + out_len]
    a = Args()
    a.key, a.key_stride_words, a.nonce, a.n = _p(k), stride // 4, _p(nn), n
    a.in_, a.pt_off, a.out = in_view.ctypes.data, _p(off), out_view.ctypes.data if out_len else out_keep.ctypes.data + base + guard
    keep = [None]
    if aads is not None:
        keep = _blob(aads, 3, 1)
        a.aad, a.aad_off = keep[1].ctypes.data if len(keep[1]) else keep[0].ctypes.data, _p(keep[2])
    ok = np.full(n + 2, 7, np.uint8)
    if not seal:
        a.ok = _p(ok)
    assert hs.hs_ascon_call(mode, int(seal), C.addressof(a)) == 0
    b = out_keep.view(np.uint8)
    assert (b[:base + guard] == 0xA5).all() and (b[base + guard + out_len:] == 0xA5).all() and (out_view[:lead] == 0xA5).all()
    assert (ok[n:] == 7).all()
    rows = [out_view[int(off[j]) + pad_out * j:int(off[j + 1]) + pad_out * (j + 1)].tobytes() for j in range(n)]
    return rows if seal else (rows, [int(x) for x in ok[:n]])


def test_the_permutation(hs):
    rng = np.random.default_rng(1)
    for rounds in (12, 8, 6):
        s = rng.integers(0, 1 << 63, 5, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5, dtype=np.uint64)
        want = [int(x) for x in s]
        ascon.perm(rounds, want)
        hs.hs_ascon_perm(rounds, _p(s))
        assert [int(x) for x in s] == want


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("base", [0, 1])
def test_every_vector_in_one_call(hs, name, base):
    mode = ascon.MODES[name]
    key, nonce, vs = vectors(name)
    pts, ads, cts = ([v[j] for v in vs] for j in range(3))
    nonces = [nonce] * len(vs)
    assert sim(hs, mode, True, key, nonces, pts, ads, base=base) == cts
    assert sim(hs, mode, False, key, nonces, cts, ads, base=base) == (pts, [1] * len(vs))


@pytest.mark.parametrize("name", NAMES)
def test_a_ragged_batch_with_distinct_keys(hs, name):
    mode = ascon.MODES[name]
    ks = ascon.key_size(mode)
    rng = np.random.default_rng(7)
    pl = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 1350, 12, 0]
    al = [0, 1, 8, 13, 16, 17, 40, 0, 1, 8, 13, 16, 17, 40, 5]
    n = len(pl)
    keys, nonces = [rng.bytes(ks) for _ in range(n)], [rng.bytes(16) for _ in range(n)]
    pts, ads = [rng.bytes(x) for x in pl], [rng.bytes(x) for x in al]
    want = [ascon.seal(mode, keys[j], nonces[j], pts[j], ads[j]) for j in range(n)]
    for base, lead, stride in ((0, 0, ks), (1, 5, 32), (3, 4, ks)):
        assert sim(hs, mode, True, keys, nonces, pts, ads, key_stride=stride, lead=lead, base=base) == want
        assert sim(hs, mode, False, keys, nonces, want, ads, key_stride=stride, lead=lead, base=base) == (pts, [1] * n)
    # one key for the batch = the same key in every row
    same = [ascon.seal(mode, keys[0], nonces[j], pts[j], ads[j]) for j in range(n)]
    assert sim(hs, mode, True, keys[0], nonces, pts, ads) == same == sim(hs, mode, True, [keys[0]] * n, nonces, pts, ads)
    # no aad blob
    assert sim(hs, mode, True, keys, nonces, pts) == [ascon.seal(mode, keys[j], nonces[j], pts[j]) for j in range(n)]
    # failure masks: a tag bit, a ct bit, an aad bit, another nonce
    bad_ct, bad_ad, bad_nonce = list(want), list(ads), list(nonces)
    bad_ct[0] = want[0][:-16] + flip(want[0][-16:], 77)
    bad_ct[12] = flip(want[12], 8 * 700 + 3)
    bad_ad[5] = flip(ads[5], 9)
    bad_nonce[14] = flip(nonces[14], 100)
    got, ok = sim(hs, mode, False, keys, bad_nonce, bad_ct, bad_ad, lead=2, base=1)
    failed = (0, 5, 12, 14)
    assert ok == [0 if j in failed else 1 for j in range(n)]
    assert got == [bytes(len(pts[j])) if j in failed else pts[j] for j in range(n)]


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "ascon_hostsim_san"), "-DASCON_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "ascon_hostsim: ok" in r.stdout, r.stdout[-3000:]
