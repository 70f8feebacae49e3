"""HPKE DHKEM over X25519 / HKDF-SHA256 (0x20) and X448 / HKDF-SHA512 (0x21) on the GPU against the RFC 9180 vectors of the reference
and the checker tests/hpke_dhkem.py; the batch SHA-256 primitive against hashlib."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import hpke_dhkem as hp
from conftest import hx, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = load_golden("hpke_dhkem.json.gz")
KEMS = [0x20, 0x21]
N_PARITY = 130   # two full wavefronts and a ragged third; Python's ladders cost milliseconds per item
BAD_AT = (0, 63, 64)


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


def _rows(items, n):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, n).copy()


def _b(a):
    return [bytes(r) for r in a]


_REF = {}


def reference(kem):
    """the checker on N_PARITY random items, computed once per KEM and shared (read-only) by the tests below"""
    if kem not in _REF:
        k = hp.Kem(kem)
        rng = np.random.default_rng(0x9180 + kem)
        d = {name: rng.integers(0, 256, (N_PARITY, k.N), dtype=np.uint8) for name in ("ikmR", "ikmS", "ikmE")}
        kr, ks = [k.derive_keypair(bytes(r)) for r in d["ikmR"]], [k.derive_keypair(bytes(r)) for r in d["ikmS"]]
        d["skR"], d["pkR"] = _rows([a for a, _ in kr], k.N), _rows([b for _, b in kr], k.N)
        d["skS"], d["pkS"] = _rows([a for a, _ in ks], k.N), _rows([b for _, b in ks], k.N)
        base = [k.encap(bytes(p), bytes(e)) for p, e in zip(d["pkR"], d["ikmE"])]
        auth = [k.auth_encap(bytes(p), bytes(s), bytes(e), bytes(q)) for p, s, e, q in zip(d["pkR"], d["skS"], d["ikmE"], d["pkS"])]
        d["enc"], d["ss"] = _rows([a for a, _ in base], k.N), _rows([b for _, b in base], k.Nh)
        d["aenc"], d["ass"] = _rows([a for a, _ in auth], k.N), _rows([b for _, b in auth], k.Nh)
        for v in d.values():
            v.setflags(write=False)
        _REF[kem] = d
    return _REF[kem]


# ---- the RFC 9180 vectors through the host-buffer calls -------------------------------------------------------------------------
@pytest.mark.parametrize("kem", KEMS)
def test_rfc9180_vectors(api, kem):
    k = hp.Kem(kem)
    vs = [v for v in VECTORS if v["kem_id"] == kem]
    assert len(vs) == 32
    col = lambda name, sub=vs: _rows([hx(v[name]) for v in sub], len(hx(sub[0][name])))
    for who in "ER":
        sk, pk = api.hpke_dhkem_derive_keypair(kem, col("ikm" + who))
        assert (sk == col("sk%sm" % who)).all() and (pk == col("pk%sm" % who)).all()
    base, auth = [v for v in vs if v["mode"] in (0, 1)], [v for v in vs if v["mode"] in (2, 3)]
    assert len(base) == 16 and len(auth) == 16
    enc, ss, ok = api.hpke_dhkem_encap(kem, col("pkRm", base), col("ikmE", base))
    assert (enc == col("enc", base)).all() and (ss == col("shared_secret", base)).all() and ok.all()
    for pk in (None, col("pkRm", base)):
        ss, ok = api.hpke_dhkem_decap(kem, col("skRm", base), col("enc", base), pkR=pk)
        assert (ss == col("shared_secret", base)).all() and ok.all()
    sk, pk = api.hpke_dhkem_derive_keypair(kem, col("ikmS", auth))
    assert (sk == col("skSm", auth)).all() and (pk == col("pkSm", auth)).all()
    for pk in (None, col("pkSm", auth)):
        enc, ss, ok = api.hpke_dhkem_auth_encap(kem, col("pkRm", auth), col("skSm", auth), col("ikmE", auth), pkS=pk)
        assert (enc == col("enc", auth)).all() and (ss == col("shared_secret", auth)).all() and ok.all()
    for pk in (None, col("pkRm", auth)):
        ss, ok = api.hpke_dhkem_auth_decap(kem, col("skRm", auth), col("enc", auth), col("pkSm", auth), pkR=pk)
        assert (ss == col("shared_secret", auth)).all() and ok.all()


# ---- parity with the checker at n = 130, every operation ------------------------------------------------------------------------
@pytest.mark.parametrize("kem", KEMS)
@pytest.mark.parametrize("op", ["derive_keypair", "encap", "decap", "auth_encap", "auth_decap"])
def test_parity_with_the_checker(api, kem, op):
    d = reference(kem)
    if op == "derive_keypair":
        sk, pk = api.hpke_dhkem_derive_keypair(kem, d["ikmR"])
        assert (sk == d["skR"]).all() and (pk == d["pkR"]).all()
    elif op == "encap":
        enc, ss, ok = api.hpke_dhkem_encap(kem, d["pkR"], d["ikmE"])
        assert (enc == d["enc"]).all() and (ss == d["ss"]).all() and ok.all()
    elif op == "decap":
        ss, ok = api.hpke_dhkem_decap(kem, d["skR"], d["enc"])
        assert (ss == d["ss"]).all() and ok.all()
    elif op == "auth_encap":
        enc, ss, ok = api.hpke_dhkem_auth_encap(kem, d["pkR"], d["skS"], d["ikmE"])
        assert (enc == d["aenc"]).all() and (ss == d["ass"]).all() and ok.all()
    else:
        ss, ok = api.hpke_dhkem_auth_decap(kem, d["skR"], d["aenc"], d["pkS"])
        assert (ss == d["ass"]).all() and ok.all()


@pytest.mark.parametrize("kem", KEMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_round_trips(api, kem, n):
    d = reference(kem)
    skR, pkR, skS, pkS, ikmE = (d[x][:n] for x in ("skR", "pkR", "skS", "pkS", "ikmE"))
    enc, ss, ok = api.hpke_dhkem_encap(kem, pkR, ikmE)
    ss2, ok2 = api.hpke_dhkem_decap(kem, skR, enc)
    assert enc.shape == (n, hp.Kem(kem).N) and (ss == ss2).all() and (ss == d["ss"][:n]).all() and ok.all() and ok2.all()
    enc, ss, ok = api.hpke_dhkem_auth_encap(kem, pkR, skS, ikmE)
    ss2, ok2 = api.hpke_dhkem_auth_decap(kem, skR, enc, pkS)
    assert (ss == ss2).all() and (ss == d["ass"][:n]).all() and ok.all() and ok2.all()


# ---- low-order points: ok = 0 and zero rows for those items, every other item unchanged -----------------------------------------
@pytest.mark.parametrize("kem", KEMS)
def test_low_order_points_in_a_batch(api, kem):
    d = reference(kem)
    k = hp.Kem(kem)
    pts = hp.low_order_points(kem)
    good = np.ones(N_PARITY, bool)
    good[list(BAD_AT)] = False

    def poisoned(rows, shift):
        a = rows.copy()
        for j, at in enumerate(BAD_AT):
            a[at] = np.frombuffer(pts[(j + shift) % len(pts)], np.uint8)
        return a

    enc, ss, ok = api.hpke_dhkem_encap(kem, poisoned(d["pkR"], 0), d["ikmE"])
    assert (ok == good).all() and not enc[~good].any() and not ss[~good].any()
    assert (enc[good] == d["enc"][good]).all() and (ss[good] == d["ss"][good]).all()
    enc, ss, ok = api.hpke_dhkem_auth_encap(kem, poisoned(d["pkR"], 1), d["skS"], d["ikmE"])
    assert (ok == good).all() and not enc[~good].any() and not ss[~good].any()
    assert (enc[good] == d["aenc"][good]).all() and (ss[good] == d["ass"][good]).all()
    ss, ok = api.hpke_dhkem_decap(kem, d["skR"], poisoned(d["enc"], 2))
    assert (ok == good).all() and not ss[~good].any() and (ss[good] == d["ss"][good]).all()
    ss, ok = api.hpke_dhkem_auth_decap(kem, d["skR"], d["aenc"], poisoned(d["pkS"], 3))
    assert (ok == good).all() and not ss[~good].any() and (ss[good] == d["ass"][good]).all()
    ss, ok = api.hpke_dhkem_auth_decap(kem, d["skR"], poisoned(d["aenc"], 4), d["pkS"])
    assert (ok == good).all() and not ss[~good].any() and (ss[good] == d["ass"][good]).all()


def test_bit_255_of_an_x25519_public_key_enters_kemctx(api):
    d = reference(0x20)
    k = hp.Kem(0x20)
    n = 8
    pkR = d["pkR"][:n].copy()
    pkR[:, 31] |= 0x80
    enc, ss, ok = api.hpke_dhkem_encap(0x20, pkR, d["ikmE"][:n])
    want = [k.encap(bytes(p), bytes(e)) for p, e in zip(pkR, d["ikmE"][:n])]
    assert _b(enc) == [a for a, _ in want] and _b(ss) == [b for _, b in want] and ok.all()
    assert (enc == d["enc"][:n]).all() and not (ss == d["ss"][:n]).all(axis=1).any()   # the same point, another kemCtx
    ss2, _ = api.hpke_dhkem_decap(0x20, d["skR"][:n], enc, pkR=pkR)
    assert (ss2 == ss).all()


@pytest.mark.parametrize("kem", KEMS)
def test_own_public_key_given_or_computed(api, kem):
    d = reference(kem)
    a = api.hpke_dhkem_decap(kem, d["skR"], d["enc"])
    b = api.hpke_dhkem_decap(kem, d["skR"], d["enc"], pkR=d["pkR"])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    a = api.hpke_dhkem_auth_encap(kem, d["pkR"], d["skS"], d["ikmE"])
    b = api.hpke_dhkem_auth_encap(kem, d["pkR"], d["skS"], d["ikmE"], pkS=d["pkS"])
    assert all((x == y).all() for x, y in zip(a, b))
    a = api.hpke_dhkem_auth_decap(kem, d["skR"], d["aenc"], d["pkS"])
    b = api.hpke_dhkem_auth_decap(kem, d["skR"], d["aenc"], d["pkS"], pkR=d["pkR"])
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


# ---- the _dev forms on torch tensors, on a stream of the caller's ---------------------------------------------------------------
@pytest.mark.parametrize("kem", KEMS)
def test_dev_forms_on_a_side_stream(kem):
    import torch
    from circl_amd import _native as nat
    from circl_amd import device as dev
    d = reference(kem)
    t = {name: torch.from_numpy(np.array(d[name])).cuda() for name in ("ikmR", "ikmS", "ikmE", "skR", "pkR", "skS", "pkS")}
    h = dev.HpkeDhkemDevice(kem)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sk, pk = h.derive_keypair(t["ikmR"])
        enc, ss, ok = h.encap(t["pkR"], t["ikmE"])
        ss2, ok2 = h.decap(t["skR"], enc)
        aenc, ass, aok = h.auth_encap(t["pkR"], t["skS"], t["ikmE"], pkS=t["pkS"])
        ass2, aok2 = h.auth_decap(t["skR"], aenc, t["pkS"])
    st.synchronize()
    assert (sk.cpu().numpy() == d["skR"]).all() and (pk.cpu().numpy() == d["pkR"]).all()
    assert (enc.cpu().numpy() == d["enc"]).all() and (ss.cpu().numpy() == d["ss"]).all() and (ss2.cpu().numpy() == d["ss"]).all()
    assert (aenc.cpu().numpy() == d["aenc"]).all() and (ass.cpu().numpy() == d["ass"]).all() and (ass2.cpu().numpy() == d["ass"]).all()
    assert all(bool(x.all()) for x in (ok, ok2, aok, aok2))
    # a misaligned pointer is refused
    raw = torch.zeros(N_PARITY * h.N + 8, dtype=torch.uint8, device="cuda")
    rc = h.L.circl_hip_hpke_dhkem_encap_dev(kem, raw.data_ptr() + 1, t["ikmE"].data_ptr(), enc.data_ptr(), ss.data_ptr(), ok.data_ptr(), N_PARITY, None)
    assert rc == nat.EWORKSPACE
    torch.cuda.synchronize()


# ---- a second pipeline chunk (CIRCL_HIP_HOST_CHUNK is read once per process) and every device ------------------------------------
@pytest.mark.parametrize("kem,chunk,device", [(0x20, "256", 0), (0x21, "256", 0), (0x20, None, -1)])
def test_chunk_boundary_and_all_devices(api, tmp_path, kem, chunk, device):
    d = reference(kem)
    k = hp.Kem(kem)
    n = 300
    rng = np.random.default_rng(300 + kem)
    ikm = {name: np.concatenate([d[name], rng.integers(0, 256, (n - N_PARITY, k.N), dtype=np.uint8)]) for name in ("ikmR", "ikmS", "ikmE")}
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **ikm)
    env = dict(os.environ)
    env.pop("CIRCL_HIP_HOST_CHUNK", None)
    if chunk:
        env["CIRCL_HIP_HOST_CHUNK"] = str(int(chunk).bit_length() - 1)   # the knob is the chunk's log2 (8..24; anything else = the default)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hpke_worker.py"), hex(kem), str(device), src, dst], check=True, env=env, timeout=300)
    o = np.load(dst)
    for name in ("skR", "pkR", "skS", "pkS", "enc", "ss", "aenc", "ass"):     # the first 130 items against the checker
        assert (o[name][:N_PARITY] == d[name]).all(), name
    assert o["ok"].all() and o["ok2"].all() and o["aok"].all() and o["aok2"].all()
    assert (o["ss2"] == o["ss"]).all() and (o["ass2"] == o["ass"]).all()
    # the rest (items 130..299, across the chunk boundary at 256) against this process's own run with the default chunk
    enc, ss, _ = api.hpke_dhkem_encap(kem, o["pkR"], ikm["ikmE"])
    aenc, ass, _ = api.hpke_dhkem_auth_encap(kem, o["pkR"], o["skS"], ikm["ikmE"])
    assert (enc == o["enc"]).all() and (ss == o["ss"]).all() and (aenc == o["aenc"]).all() and (ass == o["ass"]).all()
    for i in (255, 256, 299):                                                     # and the checker at the boundary itself
        assert k.encap(bytes(o["pkR"][i]), bytes(ikm["ikmE"][i])) == (bytes(o["enc"][i]), bytes(o["ss"][i]))


# ---- batch SHA-256 ----------------------------------------------------------------------------------------------------------------
def test_sha256_against_hashlib(api):
    rng = np.random.default_rng(256)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 55, 56, 63, 64, 119, 120, 1000)]
    out = api.sha256(msgs)
    assert _b(out) == [hashlib.sha256(m).digest() for m in msgs]
    assert api.sha256([]).shape == (0, 32)
