"""CPU-side checks of the HPKE context device source: hkdf_stream_dev.h, chacha20poly1305_dev.h and the item functions of
hpke_kernels.h compiled for the host (tests/hostsim/hpke_ctx_hostsim.hip) against hmac and the checker tests/hpke_ctx.py on the
RFC 9180 vectors, and the same source as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import hashlib
import hmac
import os
import subprocess

import numpy as np
import pytest

import hpke_ctx as hc
from conftest import hx, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = load_golden("hpke_ctx.json.gz")
SRC = os.path.join(ROOT, "tests", "hostsim", "hpke_ctx_hostsim.hip")
vp, u64 = C.c_void_p, C.c_uint64


class SetupArgs(C.Structure):  # hpke_kernels.h SetupArgs
    _fields_ = [(f, vp) for f in ("pkR", "ikmE", "skR", "skS", "pkS", "enc_out", "enc_in", "info", "psk", "psk_id", "info_off", "psk_off", "psk_id_off", "ok")] + \
               [(f, C.c_int) for f in ("kem", "kdf", "aead", "mode", "what")] + \
               [("ctx", vp), ("ctx_stride_words", C.c_size_t), ("inp", vp), ("aad", vp), ("pt_off", vp), ("aad_off", vp), ("out", vp),
                ("exp", vp), ("exp_off", vp), ("L", C.c_uint32), ("exp_out", vp), ("n", C.c_size_t)]


class AeadArgs(C.Structure):
    _fields_ = [("ctx", vp), ("ctx_stride_words", C.c_size_t), ("seq", vp), ("inp", vp), ("aad", vp), ("pt_off", vp), ("aad_off", vp), ("out", vp),
                ("ok", vp), ("n", C.c_size_t)]


class ExportArgs(C.Structure):
    _fields_ = [("ctx", vp), ("ctx_stride_words", C.c_size_t), ("kem", C.c_int), ("kdf", C.c_int), ("aead", C.c_int), ("exp", vp), ("exp_off", vp),
                ("L", C.c_uint32), ("out", vp), ("n", C.c_size_t)]


def _stale(out):
    from circl_amd import build
    deps = [SRC] + [os.path.join(build.CSRC, h) for h in os.listdir(build.CSRC) if h.endswith(".h")]
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


def _hipcc(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def hs():
    L = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libhpke_ctx_hostsim.so"), "-shared", "-fPIC"))
    L.hs_hmac_stream.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_uint32, vp, u64, vp, C.c_uint32]
    L.hs_labeled_expand_stream.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_uint32, vp, vp, u64]
    L.hs_poly1305.argtypes = [vp, vp, vp, u64]
    L.hs_setup_item.argtypes = [C.c_int, vp, u64]
    L.hs_aead_item.argtypes = [C.c_int, vp, u64]
    L.hs_export_item.argtypes = [vp, u64]
    return L


def _a(b, dtype=np.uint8):
    """a fresh array holding b (never empty, so that it has an address)"""
    a = np.zeros(max(1, -(-len(b) // np.dtype(dtype).itemsize)), dtype)
    a.view(np.uint8)[:len(b)] = np.frombuffer(b, np.uint8)
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)   # (keeps the array alive for the call)


class Rag:
    """one item's (or several items') ragged input: blob + offsets"""

    def __init__(self, items):
        self.blob = _a(b"".join(items))
        self.off = np.cumsum([0] + [len(x) for x in items]).astype(np.uint64)


@pytest.mark.parametrize("kdf", [1, 3])
def test_hmac_at_every_message_length(hs, kdf):
    h = hc.HASHES[kdf]
    nh = h().digest_size
    rng = np.random.default_rng(kdf)
    for n in range(301):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        key = rng.integers(0, 256, nh, dtype=np.uint8).tobytes()
        cut1, cut2 = n // 3, n - n // 4       # the three ranges split the message differently at every length
        a, b, c = _a(msg[:cut1]), _a(msg[cut1:cut2]), _a(msg[cut2:])
        out = np.zeros(nh // 4, np.uint32)
        hs.hs_hmac_stream(kdf, _p(out), _p(_a(key, np.uint32)), nh // 4, _p(a), cut1, _p(b), cut2 - cut1, _p(c), n - cut2)
        assert out.tobytes() == hmac.new(key, msg, h).digest(), n
        if n % 50 == 0:    # the zero key of an Extract with the empty salt
            hs.hs_hmac_stream(kdf, _p(out), None, 0, None, 0, _p(_a(msg)), n, None, 0)
            assert out.tobytes() == hmac.new(bytes(nh), msg, h).digest(), n


@pytest.mark.parametrize("kdf", [1, 3])
def test_expand_lengths(hs, kdf):
    s = hc.Suite(0x20, kdf, 3)
    rng = np.random.default_rng(kdf + 10)
    prk = rng.integers(0, 256, s.Nh, dtype=np.uint8).tobytes()
    for L in (1, s.Nh - 1, s.Nh, s.Nh + 1, 2 * s.Nh + 5, 255 * s.Nh):
        for il in (0, 1, 150):
            info = rng.integers(0, 256, il, dtype=np.uint8).tobytes()
            out = np.full(L + 8, 0xa5, np.uint8)
            hs.hs_labeled_expand_stream(0x20, kdf, 3, _p(out), L, _p(_a(prk, np.uint32)), _p(_a(info)), il)
            assert out[:L].tobytes() == s.labeled_expand(prk, b"sec", info, L), (L, il)
            assert (out[L:] == 0xa5).all()


def _poly(hs, key, msg):
    tag = np.zeros(4, np.uint32)
    hs.hs_poly1305(_p(tag), _p(_a(key, np.uint32)), _p(_a(msg)), len(msg))
    return tag.tobytes()


def test_poly1305_final_reduction(hs):
    one, two = (1).to_bytes(16, "little") + bytes(16), (2).to_bytes(16, "little") + bytes(16)
    assert _poly(hs, one, b"\xff" * 32) == (3).to_bytes(16, "little")     # h = 2^130 - 2 >= p before the last subtraction
    for key in (one, two):
        for msg in (b"\xff" * 32, b"\xff" * 16):
            assert _poly(hs, key, msg) == hc.poly1305(key, msg), (key[:1], len(msg))


def test_poly1305_random_messages(hs):
    rng = np.random.default_rng(1305)
    for n in range(0, 100):
        key, msg = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert _poly(hs, key, msg) == hc.poly1305(key, msg), n
    key = b"\xff" * 32                                                       # the largest r and s
    assert _poly(hs, key, b"\xff" * 64) == hc.poly1305(key, b"\xff" * 64)


class Item:
    """one HPKE item through the item functions of hpke_kernels.h, on the host"""

    def __init__(self, hs, v):
        self.hs, self.v = hs, v
        self.kem, self.kdf, self.aead_id, self.mode = v["kem_id"], v["kdf_id"], v["aead_id"], v["mode"]
        self.N = 32 if self.kem == 0x20 else 56
        self.cw = 12 + hc.HASHES[self.kdf]().digest_size // 4
        self.keep = []

    def _k(self, name):
        a = _a(hx(self.v[name]), np.uint32) if name in self.v else None
        self.keep.append(a)
        return _p(a)

    def _rag(self, a, blob, off, data):
        if data:
            r = Rag([data])
            self.keep.append(r)
            setattr(a, blob, _p(r.blob))
            setattr(a, off, _p(r.off))

    def setup(self, sender, what=0, **kw):
        v, a = self.v, SetupArgs()
        auth = self.mode in (2, 3)
        if sender:
            self.enc = np.full(self.N // 4, 0xa5a5a5a5, np.uint32)
            a.pkR, a.ikmE, a.skS, a.enc_out = self._k("pkRm"), self._k("ikmE"), self._k("skSm") if auth else None, _p(self.enc)
        else:
            a.skR, a.enc_in, a.pkS = self._k("skRm"), self._k("enc"), self._k("pkSm") if auth else None
        self._rag(a, "info", "info_off", hx(v["info"]))
        self._rag(a, "psk", "psk_off", hx(v.get("psk", "")))
        self._rag(a, "psk_id", "psk_id_off", hx(v.get("psk_id", "")))
        ok = np.full(1, 7, np.uint8)
        ctx = np.full(self.cw, 0xa5a5a5a5, np.uint32)
        a.ok, a.kem, a.kdf, a.aead, a.mode, a.what, a.ctx, a.ctx_stride_words, a.n = _p(ok), self.kem, self.kdf, self.aead_id, self.mode, what, _p(ctx), self.cw, 1
        out = None
        if what == 1:
            inp, pt_len = kw["inp"], kw["pt_len"]
            buf, off = _a(inp), np.array([0, pt_len], np.uint64)
            out = np.full(pt_len + (16 if sender else 0) + 4, 0xa5, np.uint8)
            self._rag(a, "aad", "aad_off", kw["aad"])
            a.inp, a.pt_off, a.out = _p(buf), _p(off), _p(out)
            out = out[:-4]
        elif what == 2:
            self._rag(a, "exp", "exp_off", kw["exp"])
            out = np.full(kw["L"], 0xa5, np.uint8)
            a.L, a.exp_out = kw["L"], _p(out)
        self.hs.hs_setup_item(int(sender), C.addressof(a), 0)
        return ctx.tobytes(), int(ok[0]), None if out is None else out.tobytes()

    def aead(self, seal, ctx, seq, inp, pt_len, aad):
        a = AeadArgs()
        row, sq, buf, off = _a(ctx, np.uint32), np.array([seq], np.uint64), _a(inp), np.array([0, pt_len], np.uint64)
        out, ok = np.full(pt_len + (16 if seal else 0), 0xa5, np.uint8), np.full(1, 7, np.uint8)
        self._rag(a, "aad", "aad_off", aad)
        a.ctx, a.ctx_stride_words, a.seq, a.inp, a.pt_off, a.out, a.ok, a.n = _p(row), self.cw, _p(sq), _p(buf), _p(off), _p(out), _p(ok), 1
        self.hs.hs_aead_item(int(seal), C.addressof(a), 0)
        return out.tobytes(), int(ok[0])

    def export(self, ctx, exp, L):
        a = ExportArgs()
        row, out = _a(ctx, np.uint32), np.full(L, 0xa5, np.uint8)
        self._rag(a, "exp", "exp_off", exp)
        a.ctx, a.ctx_stride_words, a.kem, a.kdf, a.aead, a.L, a.out, a.n = _p(row), self.cw, self.kem, self.kdf, self.aead_id, L, _p(out), 1
        self.hs.hs_export_item(C.addressof(a), 0)
        return out.tobytes()


@pytest.mark.parametrize("kem", [0x20, 0x21])
def test_the_rfc9180_vectors(hs, kem):
    vs = [v for v in VECTORS if v["kem_id"] == kem]
    assert len(vs) == 16
    for v in vs:
        it = Item(hs, v)
        want = hx(v["key"]).ljust(32, b"\0") + hx(v["base_nonce"]).ljust(12, b"\0") + bytes(4) + hx(v["exporter_secret"])
        ctx, ok, _ = it.setup(True)
        assert (ctx, ok, it.enc.tobytes()) == (want, 1, hx(v["enc"]))
        assert it.setup(False)[:2] == (want, 1)
        for e in v["encryptions"]:
            pt, aad, ct = hx(e["pt"]), hx(e["aad"]), hx(e["ct"])
            assert it.aead(True, ctx, e["seq"], pt, len(pt), aad)[0] == ct
            assert it.aead(False, ctx, e["seq"], ct, len(pt), aad) == (pt, 1)
            assert it.aead(False, ctx, e["seq"] + 1, ct, len(pt), aad) == (bytes(len(pt)), 0)
            if e["seq"] == 0:   # the single-shot forms
                assert it.setup(True, 1, inp=pt, pt_len=len(pt), aad=aad)[1:] == (1, ct)
                assert it.setup(False, 1, inp=ct, pt_len=len(pt), aad=aad)[1:] == (1, pt)
                bad = bytes([ct[0] ^ 1]) + ct[1:]
                assert it.setup(False, 1, inp=bad, pt_len=len(pt), aad=aad)[1:] == (0, bytes(len(pt)))
        for x in v["exports"]:
            exp, val = hx(x["exporter_context"]), hx(x["exported_value"])
            assert it.export(ctx, exp, x["L"]) == val
            assert it.setup(True, 2, exp=exp, L=x["L"])[1:] == (1, val)
            assert it.setup(False, 2, exp=exp, L=x["L"])[1:] == (1, val)


def test_failures_give_zero_rows(hs):
    import hpke_dhkem as hp
    v = dict(next(v for v in VECTORS if (v["kem_id"], v["kdf_id"], v["aead_id"], v["mode"]) == (0x20, 1, 3, 1)))
    pt, aad = b"some plaintext", b"aad"
    for change in (dict(psk=""), dict(psk_id=""), dict(pkRm=hp.low_order_points(0x20)[1].hex())):
        it = Item(hs, dict(v, **change))
        ctx, ok, _ = it.setup(True)
        assert (ctx, ok, it.enc.tobytes()) == (bytes(80), 0, bytes(32)), change
        assert it.setup(True, 1, inp=pt, pt_len=len(pt), aad=aad)[1:] == (0, bytes(len(pt) + 16)), change
        assert it.setup(True, 2, exp=b"x", L=40)[1:] == (0, bytes(40)), change
        assert it.enc.tobytes() == bytes(32)
    it = Item(hs, dict(v, psk=""))
    assert it.setup(False)[:2] == (bytes(80), 0)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: byte-ragged reads on blobs of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "hpke_ctx_hostsim_san"), "-DHPKE_CTX_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "hpke_ctx_hostsim: ok" in r.stdout, r.stdout[-3000:]
