"""CPU-side checks of the FrodoKEM device source: circl_amd/csrc/frodo_dev.h compiled for the host (tests/hostsim/frodo_hostsim.hip)
against the checker of tests/frodo.py -- the sampler over all 65536 inputs, pack15 / unpack15, encode / decode, the unaligned row
readers, one row of A, and one full item of each operation (the per-item device stages as they are, the matrix kernels stood in for
by loops over the device's own row squeeze)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frodo as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hs():
    out = os.path.join(ROOT, "build", "libfrodo_hostsim.so")
    src = os.path.join(ROOT, "tests", "hostsim", "frodo_hostsim.hip")
    hdrs = [os.path.join(ROOT, "circl_amd", "csrc", h) for h in ("frodo_dev.h", "keccak_dev.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "circl_amd", "csrc"), src, "-o", out])
    L = C.CDLL(out)
    for f in ("hs_frodo_sample_pair", "hs_frodo_encode_entry", "hs_frodo_decode_entry", "hs_frodo_ld32u"):
        getattr(L, f).restype = C.c_uint32
    L.hs_frodo_sample_pair.argtypes = [C.c_uint32]
    L.hs_frodo_decode_entry.argtypes = [C.c_uint32]
    L.hs_frodo_encode_entry.argtypes = [C.c_void_p, C.c_int]
    L.hs_frodo_ld32u.argtypes = [C.c_void_p]
    L.hs_frodo_row_reader.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.hs_frodo_hash_row16.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.hs_frodo_a_row.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def item():
    """one key pair and ciphertext from the checker, computed once"""
    pk, sk = ref.keygen(bytes(range(100, 148)))
    ct, ss = ref.encaps(pk, bytes(range(16)))
    return pk, sk, ct, ss


def test_sampler_all_inputs(hs):
    x = np.arange(65536, dtype=np.uint32)
    want = ref.sample(x.astype(np.uint16)).astype(np.uint32)
    # every input in the low half with a varying high half, and the other way round: the halves do not disturb each other
    for other in (0, 1, 0x7fff, 0x8000, 0xffff, 0x1234):
        o_want = int(ref.sample(np.array([other], np.uint16))[0])
        got_lo = np.array([hs.hs_frodo_sample_pair(int(v) | (other << 16)) for v in x], np.uint32)
        assert ((got_lo & 0xffff) == want).all() and ((got_lo >> 16) == o_want).all()
        got_hi = np.array([hs.hs_frodo_sample_pair((int(v) << 16) | other) for v in x[::17]], np.uint32)
        assert ((got_hi >> 16) == want[::17]).all() and ((got_hi & 0xffff) == o_want).all()


def test_pack_unpack(hs):
    rng = np.random.default_rng(7)
    cases = [np.full(8, 0xffff, np.uint32), np.zeros(8, np.uint32), np.full(8, 0x8000, np.uint32), np.full(8, 0x7fff, np.uint32)]
    for m in range(8):
        for bit in range(16):
            v = np.zeros(8, np.uint32)
            v[m] = 1 << bit
            cases.append(v)
    cases += [rng.integers(0, 65536, 8).astype(np.uint32) for _ in range(200)]
    out, back = np.zeros(16, np.uint8), np.zeros(8, np.uint32)
    for v in cases:
        out[:] = 0xAA
        hs.hs_frodo_pack8(_p(out), _p(v))
        assert out[:15].tobytes() == ref.pack(v.astype(np.uint16)) and out[15] == 0xAA   # exactly fifteen bytes are written
        hs.hs_frodo_unpack8(_p(back), _p(out))
        assert (back == (v & ref.QMASK)).all()
    assert ref.pack(np.full(8, 0xffff, np.uint16)) == b"\xff" * 15
    # unpack of arbitrary bytes, at every byte alignment of the source
    buf = np.frombuffer(rng.bytes(64), np.uint8).copy()
    for off in range(8):
        hs.hs_frodo_unpack8(_p(back), C.c_void_p(buf.ctypes.data + off))
        assert (back == ref.unpack(buf[off:off + 15].tobytes(), 8)).all()


def test_encode_decode(hs):
    rng = np.random.default_rng(8)
    for mu in (bytes(16), b"\xff" * 16, bytes(range(16)), rng.bytes(16)):
        m4 = np.frombuffer(mu, np.uint32).copy()
        got = np.array([hs.hs_frodo_encode_entry(_p(m4), e) for e in range(64)], np.uint16)
        assert (got == ref.encode(mu)).all()
    # decode over all 2^15 values of one entry (and the bit above, which the mask drops)
    w = np.arange(65536, dtype=np.uint32)
    got = np.array([hs.hs_frodo_decode_entry(int(v)) for v in w], np.uint8)
    want = ((((w & ref.QMASK) + (1 << 12)) >> 13) & 3).astype(np.uint8)
    assert (got == want).all()
    m = np.zeros(64, np.uint16)
    m[5] = 0x7fff                                             # rounds up to 4 = 0 mod 4
    assert ref.decode(m) == bytes(16) and hs.hs_frodo_decode_entry(0x7fff) == 0 and hs.hs_frodo_decode_entry(0x6fff) == 3


def test_row_readers_at_every_alignment(hs):
    rng = np.random.default_rng(9)
    buf = np.frombuffer(rng.bytes(256), np.uint8).copy()
    base = buf.ctypes.data + (-buf.ctypes.data) % 4 + 8
    lo = base - buf.ctypes.data
    for off in range(4):
        assert hs.hs_frodo_ld32u(C.c_void_p(base + off)) == int.from_bytes(buf[lo + off: lo + off + 4].tobytes(), "little")
        for nbytes in (4, 40, 172):
            out = np.zeros(nbytes // 4, np.uint32)
            hs.hs_frodo_row_reader(_p(out), C.c_void_p(base + off), nbytes)
            assert out.tobytes() == buf[lo + off: lo + off + nbytes].tobytes()
    for nbytes in (168, 172, 336, ref.PK_BYTES):                # a whole block, one dword more, two blocks, a public key
        row = np.frombuffer(rng.bytes(nbytes + 8), np.uint8).copy()
        for off in (0, 1, 3):
            out = np.zeros(4, np.uint32)
            hs.hs_frodo_hash_row16(_p(out), C.c_void_p(row.ctypes.data + off), nbytes)
            assert out.tobytes() == ref.shake128(row[off:off + nbytes].tobytes(), 16)


def test_row_of_a(hs):
    seed_a = np.frombuffer(bytes(range(50, 66)), np.uint8).copy()
    out = np.zeros(ref.N, np.uint16)
    for i in (0, 1, 255, 256, 639):
        hs.hs_frodo_a_row(_p(out), _p(seed_a), i)
        assert (out == ref.a_row(seed_a.tobytes(), i)).all()


def test_full_items(hs, item):
    pk_w, sk_w, ct_w, ss_w = item
    seed = np.frombuffer(bytes(range(100, 148)), np.uint8).copy()
    pk, sk = np.zeros(ref.PK_BYTES, np.uint8), np.zeros(ref.SK_BYTES, np.uint8)
    hs.hs_frodo_keygen(_p(seed), _p(pk), _p(sk))
    assert pk.tobytes() == pk_w and sk.tobytes() == sk_w
    mu = np.frombuffer(bytes(range(16)), np.uint8).copy()
    ct, ss = np.zeros(ref.CT_BYTES, np.uint8), np.zeros(16, np.uint8)
    hs.hs_frodo_encaps(_p(pk), _p(mu), _p(ct), _p(ss))
    assert ct.tobytes() == ct_w and ss.tobytes() == ss_w
    ss2 = np.zeros(16, np.uint8)
    hs.hs_frodo_decaps(_p(sk), _p(ct), _p(ss2))
    assert ss2.tobytes() == ss_w
    # implicit rejection, and a key taken as stored: S words 0x8000 / 0xffff / 0x7fff, another hpk
    bad = ct.copy()
    bad[9599] ^= 0x80
    hs.hs_frodo_decaps(_p(sk), _p(bad), _p(ss2))
    assert ss2.tobytes() == ref.decaps(sk_w, bad.tobytes()) == ref.shake128(bad.tobytes() + sk_w[:16], 16)
    odd = sk.copy()
    s0 = 16 + ref.PK_BYTES
    odd[s0:s0 + 6] = np.frombuffer(b"\x00\x80\xff\xff\xff\x7f", np.uint8)
    odd[-16:] ^= 0x5A
    hs.hs_frodo_decaps(_p(odd), _p(ct), _p(ss2))
    assert ss2.tobytes() == ref.decaps(odd.tobytes(), ct_w)
