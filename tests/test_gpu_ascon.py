"""Batch Ascon128 / Ascon128a / Ascon80pq on the GPU, host and _dev forms, against the reference's vectors (tests/golden/ascon.json.gz) and
the checker tests/ascon.py: every vector in one call, a ragged batch with distinct keys and nonces at odd offsets, failure masks, the
bytes around the output blobs, all-empty plaintexts, and the host pipeline's chunks, shards and copy routes (tests/ascon_worker.py)."""
import ctypes as C

import numpy as np
import pytest

import ascon
from test_oracle_ascon import flip, vectors

pytestmark = pytest.mark.gpu
N = 130            # two full wavefronts and a two-lane tail
GUARD, FILL = 64, 0xA5
NAMES = sorted(ascon.MODES)
FORMS = ["host", "dev"]
PT_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 1350)
AAD_LENS = (0, 1, 8, 13, 16, 17, 40)
vp = C.c_void_p


@pytest.fixture(scope="module")
def L():
    from circl_amd import _native as nat
    return nat.lib()


def _cuda(a):
    import torch
    torch.cuda.set_device(0)
    return torch.from_numpy(a).cuda()


class Buf:
    """bytes for one argument of either form: a host array, or its copy on the device"""

    def __init__(self, form, a):
        self.host = np.array(a)      # (a copy: contiguous and writable)
        self.t = _cuda(self.host.view(np.uint8).reshape(-1)) if form == "dev" else None

    def ptr(self, at=0):
        return vp((self.t.data_ptr() if self.t is not None else self.host.ctypes.data) + at)

    def bytes(self):
        return self.t.cpu().numpy() if self.t is not None else self.host.view(np.uint8).reshape(-1)


def call(L, form, mode, seal, keys, nonces, texts, aads=None, stride=None, lead=0, base=0, want_ok=True, no_blob=False):
    """One call of circl_hip_ascon_seal / _open in either form.  keys: one key (stride 0) or a list, `stride` bytes apart; texts:
    plaintexts (Seal) or ciphertexts (Open); lead: pt_off[0]; base: what the blobs' addresses are past a 256-byte boundary.  no_blob:
    every plaintext is empty and no plaintext blob / offsets are passed.  The output blob has GUARD sentinel bytes on each side, which
    must survive.  Returns the ciphertexts, or (plaintexts, ok)."""
    n, ks = len(texts), ascon.key_size(mode)
    shared = isinstance(keys, bytes)
    stride = 0 if shared else (stride or ks)
    krows = np.zeros((1 if shared else n, stride or ks), np.uint8)
    for j, k in enumerate([keys] if shared else keys):
        krows[j, :ks] = np.frombuffer(k, np.uint8)
    nrows = np.frombuffer(b"".join(nonces), np.uint8).reshape(n, 16)
    pts = texts if seal else [t[:-16] for t in texts]
    off = np.array([lead + sum(len(x) for x in pts[:j]) for j in range(n + 1)], np.uint64)
    pad_in, pad_out = (0, 16) if seal else (16, 0)
    src = np.zeros(base + int(off[-1]) + pad_in * n + 1, np.uint8)
    for j, t in enumerate(texts):
        at = base + int(off[j]) + pad_in * j
        src[at:at + len(t)] = np.frombuffer(t, np.uint8)
    out_len = int(off[-1]) + pad_out * n
    dst = np.full(GUARD + base + out_len + GUARD, FILL, np.uint8)
    b_key, b_nonce, b_src, b_off, b_dst = Buf(form, krows), Buf(form, nrows), Buf(form, src), Buf(form, off), Buf(form, dst)
    aad_args = [None, None]
    if aads is not None:
        aoff = np.array([3 + sum(len(x) for x in aads[:j]) for j in range(n + 1)], np.uint64)
        ab = np.zeros(1 + int(aoff[-1]) + 1, np.uint8)
        ab[4:4 + int(aoff[-1]) - 3] = np.frombuffer(b"".join(aads), np.uint8)
        b_aad, b_aoff = Buf(form, ab), Buf(form, aoff)
        aad_args = [b_aad.ptr(1), b_aoff.ptr()]
    b_ok = Buf(form, np.full(n + 2, 7, np.uint8))
    args = [mode, b_key.ptr(), stride, b_nonce.ptr(), None if no_blob and seal else b_src.ptr(base), None if no_blob else b_off.ptr(), *aad_args,
            b_dst.ptr(GUARD + base)]
    if not seal:
        args.append(b_ok.ptr() if want_ok else None)
    fn = getattr(L, "circl_hip_ascon_%s%s" % ("seal" if seal else "open", "_dev" if form == "dev" else ""))
    rc = fn(*args, n, None if form == "dev" else 0)
    assert rc == 0, (rc, L.circl_hip_last_error())
    if form == "dev":
        import torch
        torch.cuda.synchronize()
    got, ok = b_dst.bytes(), b_ok.bytes()
    body = got[GUARD + base:GUARD + base + out_len]
    assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + out_len:] == FILL).all() and (body[:lead] == FILL).all()
    assert (ok[n:] == 7).all() and (want_ok or seal or (ok == 7).all())
    rows = [body[int(off[j]) + pad_out * j:int(off[j + 1]) + pad_out * (j + 1)].tobytes() for j in range(n)]
    return rows if seal else (rows, [int(x) for x in ok[:n]])


# ---- the reference's vectors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_every_vector_in_one_call(L, form, name):
    """all 1089 vectors of a mode, one key for the batch: every pt and aad length 0..32 (both block sizes, the empty-aad skip, the
    padding word of an exact block)"""
    mode = ascon.MODES[name]
    key, nonce, vs = vectors(name)
    pts, ads, cts = ([v[j] for v in vs] for j in range(3))
    nonces = [nonce] * len(vs)
    assert call(L, form, mode, True, key, nonces, pts, ads) == cts
    assert call(L, form, mode, False, key, nonces, cts, ads) == (pts, [1] * len(vs))


@pytest.mark.parametrize("name", NAMES)
def test_the_wrappers_on_the_vectors(name):
    """hostapi.AsconCipher and device.AsconCipherDevice"""
    import torch
    from circl_amd import device, hostapi
    mode = ascon.MODES[name]
    key, nonce, vs = vectors(name)
    vs = vs[::7]
    pts, ads, cts = ([v[j] for v in vs] for j in range(3))
    n = len(vs)
    nonces = np.frombuffer(nonce * n, np.uint8).reshape(n, 16)
    c = hostapi.AsconCipher(mode, key)
    assert c.seal(nonces, pts, ads) == cts
    got, ok = c.open(nonces, cts, ads)
    assert got == pts and ok.all()
    per_item = hostapi.AsconCipher(mode, np.frombuffer(key * n, np.uint8).reshape(n, -1))
    assert per_item.seal(nonces, pts, ads) == cts
    torch.cuda.set_device(0)
    d = device.AsconCipherDevice(mode, _cuda(np.frombuffer(key, np.uint8).copy()))
    rp, ra, tn = device.Ragged(pts), device.Ragged(ads), _cuda(nonces.copy())
    ct = d.seal(tn, rp, ra)
    assert ct.cpu().numpy().tobytes() == b"".join(cts)
    pt, ok = d.open(tn, ct, rp, ra)
    assert pt.cpu().numpy()[:-1].tobytes() == b"".join(pts) and bool(ok.all())


# ---- a ragged batch with distinct keys and nonces ------------------------------------------------------------------------------------
_BATCH = {}


def batch(name):
    """130 items per mode and what the checker makes of them; computed once, shared and left unchanged.  Every plaintext length of
    PT_LENS ten times and the aad lengths of AAD_LENS in turn, both shuffled: the lanes of a wavefront have different trip counts."""
    if name not in _BATCH:
        mode = ascon.MODES[name]
        rng = np.random.default_rng(NAMES.index(name))
        pl, al = np.repeat(PT_LENS, N // len(PT_LENS)), np.resize(AAD_LENS, N)
        rng.shuffle(pl)
        rng.shuffle(al)
        keys, nonces = [rng.bytes(ascon.key_size(mode)) for _ in range(N)], [rng.bytes(16) for _ in range(N)]
        pts, ads = [rng.bytes(int(x)) for x in pl], [rng.bytes(int(x)) for x in al]
        cts = [ascon.seal(mode, keys[j], nonces[j], pts[j], ads[j]) for j in range(N)]
        _BATCH[name] = dict(mode=mode, keys=keys, nonces=nonces, pts=pts, ads=ads, cts=cts)
    return _BATCH[name]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_ragged_batch_against_the_checker(L, form, name):
    b = batch(name)
    mode, keys, nonces, pts, ads, cts = (b[k] for k in ("mode", "keys", "nonces", "pts", "ads", "cts"))
    assert len(pts) == N and {len(p) for p in pts} == set(PT_LENS) and {len(a) for a in ads} == set(AAD_LENS)
    if mode == ascon.ASCON128A:
        assert any(8 <= len(p) < 16 for p in pts)     # the partial block across the word boundary
    ks = ascon.key_size(mode)
    for stride, lead, base in ((ks, 0, 0), (32, 5, 1), (ks, 4, 8)):
        assert call(L, form, mode, True, keys, nonces, pts, ads, stride=stride, lead=lead, base=base) == cts, (stride, lead, base)
        assert call(L, form, mode, False, keys, nonces, cts, ads, stride=stride, lead=lead, base=base) == (pts, [1] * N), (stride, lead, base)
    # one key for the batch = the same key in every row
    one = call(L, form, mode, True, keys[0], nonces, pts, ads, lead=1)
    assert one == call(L, form, mode, True, [keys[0]] * N, nonces, pts, ads, stride=32)
    assert one[0] == cts[0] and one[N - 1] == ascon.seal(mode, keys[0], nonces[N - 1], pts[N - 1], ads[N - 1])
    assert call(L, form, mode, False, keys[0], nonces, one, ads, base=3) == (pts, [1] * N)
    # no aad blob
    no_aad = call(L, form, mode, True, keys, nonces, pts)
    assert [no_aad[j] for j in (0, 63, 64, 129)] == [ascon.seal(mode, keys[j], nonces[j], pts[j]) for j in (0, 63, 64, 129)]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_failure_masks(L, form, name):
    """a tag bit, a ciphertext bit, an aad bit and another nonce at both ends of both wavefronts' boundary"""
    b = batch(name)
    mode, keys, pts = b["mode"], b["keys"], list(b["pts"])
    nonces, ads, cts = list(b["nonces"]), list(b["ads"]), list(b["cts"])
    # items 63 and 64 need a ciphertext byte and an aad byte to corrupt: give them fixed ones
    pts[63], ads[64] = b"sixty-three" * 3, b"sixty-four"
    for j in (63, 64):
        cts[j] = ascon.seal(mode, keys[j], nonces[j], pts[j], ads[j])
    assert call(L, form, mode, False, keys, nonces, cts, ads) == (pts, [1] * N)
    cts[0] = cts[0][:-16] + flip(cts[0][-16:], 77)
    cts[63] = flip(cts[63], 50)
    ads[64] = flip(ads[64], 9)
    nonces[129] = flip(nonces[129], 100)
    failed = (0, 63, 64, 129)
    want = [bytes(len(pts[j])) if j in failed else pts[j] for j in range(N)]
    assert call(L, form, mode, False, keys, nonces, cts, ads, lead=3, base=1) == (want, [0 if j in failed else 1 for j in range(N)])
    got, _ = call(L, form, mode, False, keys, nonces, cts, ads, want_ok=False)      # ok = NULL
    assert got == want


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_an_open_where_every_item_fails(L, form, name):
    """every row is cleared and nothing around the blob is touched (call() checks the sentinels of every call)"""
    b = batch(name)
    wrong = [flip(k, 3) for k in b["keys"]]
    got, ok = call(L, form, b["mode"], False, wrong, b["nonces"], b["cts"], b["ads"], lead=7, base=5)
    assert ok == [0] * N and got == [bytes(len(p)) for p in b["pts"]]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("form", FORMS)
def test_empty_plaintexts_without_a_blob(L, form, name):
    b = batch(name)
    mode, keys, nonces, ads = b["mode"], b["keys"], b["nonces"], b["ads"]
    tags = call(L, form, mode, True, keys, nonces, [b""] * N, ads, no_blob=True)
    assert tags == [ascon.seal(mode, keys[j], nonces[j], b"", ads[j]) for j in range(N)] and all(len(t) == 16 for t in tags)
    assert call(L, form, mode, False, keys, nonces, tags, ads, no_blob=True) == ([b""] * N, [1] * N)
    tags[64] = flip(tags[64], 127)
    assert call(L, form, mode, False, keys, nonces, tags, ads, no_blob=True) == ([b""] * N, [0 if j == 64 else 1 for j in range(N)])


# ---- the host pipeline's routes -------------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 items at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices
SPOTS = (0, 99, 100, 199, 200, 255, 256, 299)   # both ends, both sides of the shard boundaries and of the chunk boundary


@pytest.fixture(scope="module")
def pipe(L):
    """this process's own run with the default settings -- one chunk at lo = 0 -- computed once and shared"""
    import ascon_worker as aw
    return aw.run(L, 0, N_PIPE)


def _items(flat, lens, extra=0):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [flat[int(off[j]) + extra * j:int(off[j + 1]) + extra * (j + 1)].tobytes() for j in range(len(lens))]


def _check_pipeline_run(o, base):
    """what every configuration asserts about one run of ascon_worker.run"""
    import ascon_worker as aw
    keys, nonces, pts, aads = aw.inputs(N_PIPE)
    lens = [len(x) for x in pts]
    assert lens[0] == lens[255] == lens[256] == 0 and lens[299] == 3 and lens[100] == 26
    for k in base:
        assert o[k].shape == base[k].shape and (np.asarray(o[k]) == base[k]).all(), k
    for name, mode, ks in aw.KEYINGS:
        g = lambda what: o[name + "_" + what]
        key = lambda j: keys[name][j, :ks].tobytes() if name == "a128" else keys[name].tobytes()
        assert g("ok").all() and g("pt").tobytes() == b"".join(pts), name
        assert g("ct").size == sum(lens) + 16 * N_PIPE and g("tags").size == 16 * N_PIPE
        ct, ct_noaad, tags = _items(g("ct"), lens, 16), _items(g("ct_noaad"), lens, 16), _items(g("tags"), [0] * N_PIPE, 16)
        for j in SPOTS:
            nonce = nonces[j].tobytes()
            assert ct[j] == ascon.seal(mode, key(j), nonce, pts[j], aads[j]) and ct_noaad[j] == ascon.seal(mode, key(j), nonce, pts[j]), (name, j)
            assert tags[j] == ascon.seal(mode, key(j), nonce, b"", aads[j]), (name, j)
        # forged tags: ok = 0 and zeros of the right length there, every other item intact
        assert g("fok").tolist() == [0 if j in aw.FORGED else 1 for j in range(N_PIPE)], name
        assert _items(g("fpt"), lens) == [bytes(lens[j]) if j in aw.FORGED else pts[j] for j in range(N_PIPE)], name
        assert g("tok").tolist() == [0 if j == aw.FORGED_TAG else 1 for j in range(N_PIPE)], name
    assert o["guards"].all()      # nothing was written before or behind an output


def test_pipeline_default_run_takes_the_checks(pipe):
    _check_pipeline_run(pipe, pipe)


@pytest.mark.parametrize("env,device", [({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1),
                                        ({"CIRCL_HIP_ZEROCOPY_KB": "0"}, 0)], ids=["chunks", "chunks-in-shards", "merged-copy"])
def test_pipeline_routes_agree(pipe, tmp_path, env, device):
    import os
    import subprocess
    import sys
    dst = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ascon_worker.py"), str(device), str(N_PIPE), dst], check=True,
                   env=e, timeout=300)
    _check_pipeline_run(np.load(dst), pipe)
