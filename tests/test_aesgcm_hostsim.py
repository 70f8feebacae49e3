"""CPU-side checks of the AES-GCM device source: the item functions of aesgcm_kernels.h compiled for the host
(tests/hostsim/aesgcm_hostsim.hip) on every encryption of the fixture and on a ragged batch with distinct keys against the checker
tests/aesgcm.py, one AES block against libcrypto's ECB, one GHASH product against the big-integer product, and the same source as a
stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aesgcm
from test_oracle_aesgcm import evp_ecb, flip, vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "aesgcm_hostsim.hip")
vp, sz = C.c_void_p, C.c_size_t
SIZES = aesgcm.KEY_SIZES


class Args(C.Structure):  # aesgcm_kernels.h Args
    _fields_ = [("key", vp), ("key_stride_words", sz), ("nonce", vp), ("nonce_stride_words", sz), ("seq", vp), ("in_", vp), ("aad", vp), ("pt_off", vp),
                ("aad_off", vp), ("out", vp), ("ok", vp), ("n", sz)]


def _stale(out):
    from circl_amd import build
    deps = [SRC] + [os.path.join(build.CSRC, h) for h in ("aesgcm_dev.h", "aesgcm_kernels.h", "chacha20poly1305_dev.h", "keccak_dev.h")]
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


def _hipcc(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def hs():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libaesgcm_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_aesgcm_call.argtypes = [C.c_int, C.c_int, vp]
    lib.hs_aes_encrypt_block.argtypes = [C.c_int, vp, vp, vp, C.c_int]
    lib.hs_ghash_mul.argtypes = [vp, vp, vp]
    lib.hs_ghash_mul_many.argtypes = [vp, vp, vp, sz]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(vp)


def _rows(rows, stride):
    """a fresh word-aligned array holding the rows `stride` bytes apart"""
    a = np.zeros(max(1, (len(rows) * stride + 3) // 4), np.uint32)
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


def sim(hs, seal, keys, nonces, texts, aads=None, seq=None, key_stride=None, nonce_stride=12, lead=0, base=0, guard=16):
    """One call through the host instantiation.  keys: one key (shared) or a list; nonces: one base nonce (shared, with seq) or a list.
    texts: plaintexts (seal) or ciphertexts (open).  Returns the ciphertexts, or (plaintexts, ok).  The output blob has `guard`
    sentinel bytes on each side."""
    n = len(texts)
    shared, one_nonce = isinstance(keys, bytes), isinstance(nonces, bytes)
    ks = len(keys) if shared else len(keys[0])
    stride = 0 if shared else (key_stride or ks)
    nstride = 0 if one_nonce else nonce_stride
    k, nn = _rows([keys] if shared else keys, stride or ks), _rows([nonces] if one_nonce else nonces, nstride or 12)
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
    a.key, a.key_stride_words, a.nonce, a.nonce_stride_words, a.n = _p(k), stride // 4, _p(nn), nstride // 4, n
    sq = None if seq is None else np.array(seq, np.uint64)
    a.seq = _p(sq)
    a.in_, a.pt_off, a.out = in_view.ctypes.data, _p(off), out_view.ctypes.data if out_len else out_keep.ctypes.data + base + guard
    keep = [None]
    if aads is not None:
        keep = _blob(aads, 3, 1)
        a.aad, a.aad_off = keep[1].ctypes.data if len(keep[1]) else keep[0].ctypes.data, _p(keep[2])
    ok = np.full(n + 2, 7, np.uint8)
    if not seal:
        a.ok = _p(ok)
    assert hs.hs_aesgcm_call(ks, int(seal), C.addressof(a)) == 0
    b = out_keep.view(np.uint8)
    assert (b[:base + guard] == 0xA5).all() and (b[base + guard + out_len:] == 0xA5).all() and (out_view[:lead] == 0xA5).all()
    assert (ok[n:] == 7).all()
    rows = [out_view[int(off[j]) + pad_out * j:int(off[j + 1]) + pad_out * (j + 1)].tobytes() for j in range(n)]
    return rows if seal else (rows, [int(x) for x in ok[:n]])


# ---- function level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", SIZES)
def test_one_aes_block(hs, ks):
    """256 random (key, block) pairs and the all-zero / all-ones key and block, in either slot of the two-block pass, against libcrypto's
    ECB (the checker where libcrypto is absent)"""
    try:
        import test_oracle_aesgcm as t
        L = t.libcrypto()
        want = lambda key, block: evp_ecb(L, key, block)
    except pytest.skip.Exception:
        want = lambda key, block: aesgcm.encrypt_block(aesgcm.expand_key(key), block)
    rng = np.random.default_rng(197 + ks)
    pairs = [(rng.bytes(ks), rng.bytes(16)) for _ in range(256)]
    pairs += [(bytes([a]) * ks, bytes([b]) * 16) for a in (0, 255) for b in (0, 255)]
    for j, (key, block) in enumerate(pairs):
        k, i, o = np.frombuffer(key, np.uint32).copy(), np.frombuffer(block, np.uint32).copy(), np.zeros(4, np.uint32)
        assert hs.hs_aes_encrypt_block(ks, _p(k), _p(i), _p(o), j & 1) == 0
        assert o.tobytes() == want(key, block), j
        if j >= 256:    # the fixed pairs in the other slot too
            assert hs.hs_aes_encrypt_block(ks, _p(k), _p(i), _p(o), ~j & 1) == 0 and o.tobytes() == want(key, block)
    assert aesgcm.encrypt_block(aesgcm.expand_key(pairs[0][0]), pairs[0][1]) == want(*pairs[0])


def _products(hs, pairs):
    x = np.frombuffer(b"".join(a.to_bytes(16, "big") for a, _ in pairs), np.uint8).copy()
    h = np.frombuffer(b"".join(b.to_bytes(16, "big") for _, b in pairs), np.uint8).copy()
    out = np.zeros_like(x)
    hs.hs_ghash_mul_many(_p(x), _p(h), _p(out), len(pairs))
    return [int.from_bytes(out[16 * j:16 * j + 16].tobytes(), "big") for j in range(len(pairs))]


def test_ghash_mul(hs):
    """against the big-integer product: every pair of single-bit operands, all-ones x all-ones, all-ones x every single bit (both ways),
    0, the field's one (the block 80 00 .. 00), and 1024 random pairs"""
    ones, one = (1 << 128) - 1, 1 << 127
    bits = [1 << j for j in range(128)]
    pairs = [(a, b) for a in bits for b in bits]
    pairs += [(ones, ones)] + [(ones, b) for b in bits] + [(b, ones) for b in bits]
    pairs += [(0, 0), (0, ones), (ones, 0), (one, one), (one, ones), (ones, one), (one, 0x0123456789abcdef0fedcba987654321)]
    rng = np.random.default_rng(128)
    pairs += [(int.from_bytes(rng.bytes(16), "big"), int.from_bytes(rng.bytes(16), "big")) for _ in range(1024)]
    got = _products(hs, pairs)
    for (a, b), g in zip(pairs, got):
        assert g == aesgcm.ghash_mul(a, b), (hex(a), hex(b))
    assert aesgcm.ghash_mul(one, 0x1234) == 0x1234 and aesgcm.ghash_mul(ones, 0) == 0
    # one product through the single-product entry point
    out = np.zeros(16, np.uint8)
    hs.hs_ghash_mul(_p(np.frombuffer(ones.to_bytes(16, "big"), np.uint8).copy()), _p(np.frombuffer(ones.to_bytes(16, "big"), np.uint8).copy()), _p(out))
    assert int.from_bytes(out.tobytes(), "big") == aesgcm.ghash_mul(ones, ones)


# ---- the item functions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("base", [0, 1])
def test_every_vector_in_one_call(hs, ks, base):
    vs = vectors(ks)
    keys, bases, seqs, nonces, ads, pts, cts = ([v[j] for v in vs] for j in range(7))
    assert sim(hs, True, keys, nonces, pts, ads, base=base) == cts
    assert sim(hs, False, keys, nonces, cts, ads, base=base) == (pts, [1] * len(vs))
    assert sim(hs, True, keys, bases, pts, ads, seq=seqs, base=base) == cts
    assert sim(hs, False, keys, bases, cts, ads, seq=seqs, base=base) == (pts, [1] * len(vs))


@pytest.mark.parametrize("ks", SIZES)
def test_a_ragged_batch_with_distinct_keys(hs, ks):
    rng = np.random.default_rng(7 + ks)
    pl = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 1350, 12, 0]
    al = [0, 1, 8, 13, 16, 17, 40, 0, 1, 8, 13, 16, 17, 40, 5, 33, 32, 31]
    n = len(pl)
    keys, nonces = [rng.bytes(ks) for _ in range(n)], [rng.bytes(12) for _ in range(n)]
    pts, ads = [rng.bytes(x) for x in pl], [rng.bytes(x) for x in al]
    want = [aesgcm.seal(keys[j], nonces[j], pts[j], ads[j]) for j in range(n)]
    for base, lead, stride, nstride in ((0, 0, ks, 12), (1, 5, ks + 4, 16), (3, 4, 80, 80)):
        assert sim(hs, True, keys, nonces, pts, ads, key_stride=stride, nonce_stride=nstride, lead=lead, base=base) == want
        assert sim(hs, False, keys, nonces, want, ads, key_stride=stride, nonce_stride=nstride, lead=lead, base=base) == (pts, [1] * n)
    # one key for the batch = the same key in every row
    same = [aesgcm.seal(keys[0], nonces[j], pts[j], ads[j]) for j in range(n)]
    assert sim(hs, True, keys[0], nonces, pts, ads) == same == sim(hs, True, [keys[0]] * n, nonces, pts, ads)
    # one key and one base nonce for the batch, seq = 0 .. n - 1 and far up
    for first in (0, (1 << 40) - 3):
        seq = [first + j for j in range(n)]
        run = [aesgcm.seal(keys[1], aesgcm.seq_nonce(nonces[1], seq[j]), pts[j], ads[j]) for j in range(n)]
        assert sim(hs, True, keys[1], nonces[1], pts, ads, seq=seq) == run
        assert sim(hs, False, keys[1], nonces[1], run, ads, seq=seq) == (pts, [1] * n)
    # no aad blob
    assert sim(hs, True, keys, nonces, pts) == [aesgcm.seal(keys[j], nonces[j], pts[j]) for j in range(n)]
    # failure masks: a tag bit, a ct bit, an aad bit, another nonce, another key
    bad_ct, bad_ad, bad_nonce, bad_key = list(want), list(ads), list(nonces), list(keys)
    bad_ct[0] = want[0][:-16] + flip(want[0][-16:], 77)
    bad_ct[15] = flip(want[15], 8 * 700 + 3)
    bad_ad[5] = flip(ads[5], 9)
    bad_nonce[16] = flip(nonces[16], 90)
    bad_key[9] = flip(keys[9], 8 * ks - 1)
    got, ok = sim(hs, False, bad_key, bad_nonce, bad_ct, bad_ad, lead=2, base=1)
    failed = (0, 5, 9, 15, 16)
    assert ok == [0 if j in failed else 1 for j in range(n)]
    assert got == [bytes(len(pts[j])) if j in failed else pts[j] for j in range(n)]


@pytest.mark.parametrize("ks", SIZES)
def test_the_counter_carries(hs, ks):
    """4097 bytes: counters 2 .. 258, past the low byte of the 32-bit big-endian counter"""
    rng = np.random.default_rng(4097 + ks)
    key, nonce, pts, ad = rng.bytes(ks), rng.bytes(12), [b"", rng.bytes(4097), b"x"], b"thirteen byte"
    want = [aesgcm.seal(key, nonce, p, ad) for p in pts]
    assert sim(hs, True, key, [nonce] * 3, pts, [ad] * 3) == want
    assert sim(hs, False, key, [nonce] * 3, want, [ad] * 3) == (pts, [1] * 3)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "aesgcm_hostsim_san"), "-DAESGCM_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "aesgcm_hostsim: ok" in r.stdout, r.stdout[-3000:]
