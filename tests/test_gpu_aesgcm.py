"""Batch AES-128-GCM / AES-256-GCM on the GPU, host and _dev forms, against the reference's known answers
(tests/golden/aesgcm_hpke.json.gz) and the checker tests/aesgcm.py: every vector of a key size in one call, every plaintext length
0 .. 130, the counter's carry, keys and nonces at every stride the ABI allows, failure masks, the bytes around the output blobs,
all-empty plaintexts, and the host pipeline's chunks, shards and copy routes (tests/aesgcm_worker.py)."""
import ctypes as C

import numpy as np
import pytest

import aesgcm
from test_oracle_aesgcm import flip, vectors

pytestmark = pytest.mark.gpu
N = 130            # two full wavefronts and a two-lane tail
GUARD, FILL = 64, 0xA5
SIZES = aesgcm.KEY_SIZES
FORMS = ["host", "dev"]
AAD_LENS = (0, 1, 7, 8, 13, 15, 16, 17, 31, 32, 33, 40)
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


def call(L, form, seal, keys, nonces, texts, aads=None, seq=None, stride=None, nstride=12, rows=0, lead=0, base=0, want_ok=True, no_blob=False):
    """One call of circl_hip_aesgcm_seal / _open in either form.  keys: one key (stride 0) or a list, `stride` bytes apart; nonces: one
    base nonce (stride 0; needs seq) or a list, `nstride` bytes apart; rows: both in ONE array of rows of that many bytes, key at +0
    and nonce at +32 (an array of HPKE-style context rows).  texts: plaintexts (Seal) or ciphertexts (Open); lead: pt_off[0]; base: what
    the blobs' addresses are past a 256-byte boundary.  no_blob: every plaintext is empty and no plaintext blob / offsets are passed.
    The output blob has GUARD sentinel bytes on each side, which must survive.  Returns the ciphertexts, or (plaintexts, ok)."""
    n = len(texts)
    shared, one_nonce = isinstance(keys, bytes), isinstance(nonces, bytes)
    ks = len(keys) if shared else len(keys[0])
    if rows:
        both = np.random.default_rng(rows).integers(0, 256, (n, rows), dtype=np.uint8)       # noise between and behind the fields
        for j in range(n):
            both[j, :ks] = np.frombuffer(keys[j], np.uint8)
            both[j, 32:44] = np.frombuffer(nonces[j], np.uint8)
        b_key = b_nonce = Buf(form, both)
        key_args = [b_key.ptr(), rows, b_nonce.ptr(32), rows]
    else:
        stride = 0 if shared else (stride or ks)
        nstride = 0 if one_nonce else nstride
        krows = np.zeros((1 if shared else n, stride or ks), np.uint8)
        for j, k in enumerate([keys] if shared else keys):
            krows[j, :ks] = np.frombuffer(k, np.uint8)
        nrows = np.full((1 if one_nonce else n, nstride or 12), 0x5C, np.uint8)
        for j, x in enumerate([nonces] if one_nonce else nonces):
            nrows[j, :12] = np.frombuffer(x, np.uint8)
        b_key, b_nonce = Buf(form, krows), Buf(form, nrows)
        key_args = [b_key.ptr(), stride, b_nonce.ptr(), nstride]
    b_seq = None if seq is None else Buf(form, np.array(seq, np.uint64))
    pts = texts if seal else [t[:-16] for t in texts]
    off = np.array([lead + sum(len(x) for x in pts[:j]) for j in range(n + 1)], np.uint64)
    pad_in, pad_out = (0, 16) if seal else (16, 0)
    src = np.zeros(base + int(off[-1]) + pad_in * n + 1, np.uint8)
    for j, t in enumerate(texts):
        at = base + int(off[j]) + pad_in * j
        src[at:at + len(t)] = np.frombuffer(t, np.uint8)
    out_len = int(off[-1]) + pad_out * n
    dst = np.full(GUARD + base + out_len + GUARD, FILL, np.uint8)
    b_src, b_off, b_dst = Buf(form, src), Buf(form, off), Buf(form, dst)
    aad_args = [None, None]
    if aads is not None:
        aoff = np.array([3 + sum(len(x) for x in aads[:j]) for j in range(n + 1)], np.uint64)
        ab = np.zeros(1 + int(aoff[-1]) + 1, np.uint8)
        ab[4:4 + int(aoff[-1]) - 3] = np.frombuffer(b"".join(aads), np.uint8)
        b_aad, b_aoff = Buf(form, ab), Buf(form, aoff)
        aad_args = [b_aad.ptr(1), b_aoff.ptr()]
    b_ok = Buf(form, np.full(n + 2, 7, np.uint8))
    args = [ks, *key_args, None if b_seq is None else b_seq.ptr(), None if no_blob and seal else b_src.ptr(base), None if no_blob else b_off.ptr(), *aad_args,
            b_dst.ptr(GUARD + base)]
    if not seal:
        args.append(b_ok.ptr() if want_ok else None)
    fn = getattr(L, "circl_hip_aesgcm_%s%s" % ("seal" if seal else "open", "_dev" if form == "dev" else ""))
    rc = fn(*args, n, None if form == "dev" else 0)
    assert rc == 0, (rc, L.circl_hip_last_error())
    if form == "dev":
        import torch
        torch.cuda.synchronize()
    got, ok = b_dst.bytes(), b_ok.bytes()
    body = got[GUARD + base:GUARD + base + out_len]
    assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + out_len:] == FILL).all() and (body[:lead] == FILL).all()
    assert (ok[n:] == 7).all() and (want_ok or seal or (ok == 7).all())
    rows_out = [body[int(off[j]) + pad_out * j:int(off[j + 1]) + pad_out * (j + 1)].tobytes() for j in range(n)]
    return rows_out if seal else (rows_out, [int(x) for x in ok[:n]])


# ---- the reference's known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_every_vector_in_one_call(L, form, ks):
    """all 192 encryptions under keys of one size (32 vectors x sequence numbers 0, 1, 2, 4, 255, 256): per-item keys with the explicit
    nonces, and per-item keys with base_nonce + seq"""
    vs = vectors(ks)
    keys, bases, seqs, nonces, ads, pts, cts = ([v[j] for v in vs] for j in range(7))
    assert call(L, form, True, keys, nonces, pts, ads) == cts
    assert call(L, form, False, keys, nonces, cts, ads) == (pts, [1] * len(vs))
    assert call(L, form, True, keys, bases, pts, ads, seq=seqs) == cts
    assert call(L, form, False, keys, bases, cts, ads, seq=seqs) == (pts, [1] * len(vs))


# ---- lengths, against the checker -----------------------------------------------------------------------------------------------
_BATCH = {}


def batch(ks):
    """131 items per key size and what the checker makes of them; computed once, shared and left unchanged.  Every plaintext length
    0 .. 130 (every partial final block, every boundary of a two- or four-block pass), shuffled so that the lanes of a wavefront have
    different trip counts, and the aad lengths of AAD_LENS in turn."""
    if ks not in _BATCH:
        rng = np.random.default_rng(ks)
        pl = np.arange(131)
        rng.shuffle(pl)
        al = np.resize(AAD_LENS, 131)
        keys, nonces = [rng.bytes(ks) for _ in range(131)], [rng.bytes(12) for _ in range(131)]
        pts, ads = [rng.bytes(int(x)) for x in pl], [rng.bytes(int(x)) for x in al]
        cts = [aesgcm.seal(keys[j], nonces[j], pts[j], ads[j]) for j in range(131)]
        _BATCH[ks] = dict(keys=keys, nonces=nonces, pts=pts, ads=ads, cts=cts)
    return _BATCH[ks]


@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_every_plaintext_length(L, form, ks):
    b = batch(ks)
    keys, nonces, pts, ads, cts = (b[k] for k in ("keys", "nonces", "pts", "ads", "cts"))
    assert sorted(len(p) for p in pts) == list(range(131)) and {len(a) for a in ads} == set(AAD_LENS)
    assert call(L, form, True, keys, nonces, pts, ads) == cts
    assert call(L, form, False, keys, nonces, cts, ads) == (pts, [1] * 131)
    assert call(L, form, True, keys, nonces, pts, ads, lead=5, base=1) == cts
    assert call(L, form, False, keys, nonces, cts, ads, lead=4, base=3) == (pts, [1] * 131)


@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_the_counter_carries(L, form, ks):
    """4097 bytes reach counter value 258: block 254 carries out of the low byte of the 32-bit big-endian counter.  Its neighbours in
    the wavefront have 0 and 1 bytes: lanes that finish far apart."""
    rng = np.random.default_rng(4097 + ks)
    pl = [0, 4097, 1] + [j % 3 for j in range(7)]
    keys, nonces = [rng.bytes(ks) for _ in pl], [rng.bytes(12) for _ in pl]
    pts, ads = [rng.bytes(x) for x in pl], [b"thirteen byte"] * len(pl)
    cts = [aesgcm.seal(keys[j], nonces[j], pts[j], ads[j]) for j in range(len(pl))]
    assert call(L, form, True, keys, nonces, pts, ads) == cts
    assert call(L, form, False, keys, nonces, cts, ads) == (pts, [1] * len(pl))


# ---- keys and nonces --------------------------------------------------------------------------------------------------------------
def _first(b, n=N):
    return (b[k][:n] for k in ("keys", "nonces", "pts", "ads", "cts"))


@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_key_and_nonce_strides(L, form, ks):
    keys, nonces, pts, ads, cts = _first(batch(ks))
    # distinct keys at key_bytes + 4, nonces at 16
    assert call(L, form, True, keys, nonces, pts, ads, stride=ks + 4, nstride=16, lead=5, base=1) == cts
    assert call(L, form, False, keys, nonces, cts, ads, stride=ks + 4, nstride=16, lead=4, base=8) == (pts, [1] * N)
    # an array of context rows: stride 80, the nonce at +32
    assert call(L, form, True, keys, nonces, pts, ads, rows=80) == cts
    assert call(L, form, False, keys, nonces, cts, ads, rows=80) == (pts, [1] * N)
    if ks == 32:
        assert call(L, form, True, keys, nonces, pts, ads, rows=112, base=3) == cts
    # one key for the batch = the same key in every row
    one = call(L, form, True, keys[0], nonces, pts, ads, lead=1)
    assert one == call(L, form, True, [keys[0]] * N, nonces, pts, ads, stride=32)
    assert one[0] == cts[0] and one[N - 1] == aesgcm.seal(keys[0], nonces[N - 1], pts[N - 1], ads[N - 1])
    assert call(L, form, False, keys[0], nonces, one, ads, base=3) == (pts, [1] * N)
    # one key and one base nonce for the batch, seq = 0 .. n - 1: one HPKE context sealing a run of records
    seq = list(range(N))
    run = call(L, form, True, keys[1], nonces[1], pts, ads, seq=seq)
    assert [run[j] for j in (0, 1, 63, 64, 129)] == [aesgcm.seal(keys[1], aesgcm.seq_nonce(nonces[1], j), pts[j], ads[j]) for j in (0, 1, 63, 64, 129)]
    assert call(L, form, False, keys[1], nonces[1], run, ads, seq=seq) == (pts, [1] * N)
    assert call(L, form, False, keys[1], nonces[1], run, ads, seq=[j + 1 for j in seq])[1] == [0] * N
    # sequence numbers above 2^32 with per-item base nonces
    far = [(1 << 40) - 3 + j for j in range(N)]
    got = call(L, form, True, keys, nonces, pts, ads, seq=far, nstride=16)
    assert [got[j] for j in (0, 3, 129)] == [aesgcm.seal(keys[j], aesgcm.seq_nonce(nonces[j], far[j]), pts[j], ads[j]) for j in (0, 3, 129)]
    # no aad blob
    no_aad = call(L, form, True, keys, nonces, pts)
    assert [no_aad[j] for j in (0, 63, 64, 129)] == [aesgcm.seal(keys[j], nonces[j], pts[j]) for j in (0, 63, 64, 129)]


# ---- failure masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_failure_masks(L, form, ks):
    """one flipped bit in turn of the tag, of the last ciphertext byte, of the aad, of the nonce and of the key, on a third of the items
    of the shuffled batch"""
    keys, nonces, pts, ads, cts = (list(x) for x in _first(batch(ks)))
    for j in range(0, N, 3):            # a ciphertext byte and an aad byte to corrupt, wherever the flip falls
        if not pts[j] or not ads[j]:
            pts[j], ads[j] = pts[j] or b"item %3d" % j, ads[j] or b"aad"
            cts[j] = aesgcm.seal(keys[j], nonces[j], pts[j], ads[j])
    assert call(L, form, False, keys, nonces, cts, ads) == (pts, [1] * N)
    failed = list(range(0, N, 3))
    assert {0, 63, 129} <= set(failed) and len(failed) == 44
    for k, j in enumerate(failed):
        what = k % 5
        if what == 0:
            cts[j] = cts[j][:-16] + flip(cts[j][-16:], (7 * k) % 128)
        elif what == 1:
            cts[j] = flip(cts[j], 8 * (len(pts[j]) - 1) + k % 8)
        elif what == 2:
            ads[j] = flip(ads[j], (3 * k) % (8 * len(ads[j])))
        elif what == 3:
            nonces[j] = flip(nonces[j], (11 * k) % 96)
        else:
            keys[j] = flip(keys[j], (13 * k) % (8 * ks))
    want = [bytes(len(pts[j])) if j in failed else pts[j] for j in range(N)]
    assert call(L, form, False, keys, nonces, cts, ads, lead=3, base=1) == (want, [0 if j in failed else 1 for j in range(N)])
    got, _ = call(L, form, False, keys, nonces, cts, ads, want_ok=False)      # ok = NULL
    assert got == want


@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_an_open_where_every_item_fails(L, form, ks):
    """every row is cleared and nothing around the blob is touched (call() checks the sentinels of every call)"""
    keys, nonces, pts, ads, cts = _first(batch(ks))
    wrong = [flip(k, 3) for k in keys]
    got, ok = call(L, form, False, wrong, nonces, cts, ads, lead=7, base=5)
    assert ok == [0] * N and got == [bytes(len(p)) for p in pts]


@pytest.mark.parametrize("ks", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_empty_plaintexts_without_a_blob(L, form, ks):
    keys, nonces, _, ads, _ = _first(batch(ks))
    tags = call(L, form, True, keys, nonces, [b""] * N, ads, no_blob=True)
    assert tags == [aesgcm.seal(keys[j], nonces[j], b"", ads[j]) for j in range(N)] and all(len(t) == 16 for t in tags)
    assert call(L, form, False, keys, nonces, tags, ads, no_blob=True) == ([b""] * N, [1] * N)
    tags[64] = flip(tags[64], 127)
    assert call(L, form, False, keys, nonces, tags, ads, no_blob=True) == ([b""] * N, [0 if j == 64 else 1 for j in range(N)])


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", SIZES)
def test_the_wrappers_round_trip_and_agree_with_the_checker(ks):
    """hostapi.AesGcm and device.AesGcmDevice"""
    import torch
    from circl_amd import device, hostapi
    keys, nonces, pts, ads, cts = (x[::5] for x in _first(batch(ks)))
    n = len(pts)
    nn, kk = np.frombuffer(b"".join(nonces), np.uint8).reshape(n, 12), np.frombuffer(b"".join(keys), np.uint8).reshape(n, ks)
    c = hostapi.AesGcm(kk)
    assert c.seal(nn, pts, ads) == cts
    got, ok = c.open(nn, cts, ads)
    assert got == pts and ok.all()
    one = hostapi.AesGcm(keys[0])
    run = one.seal(nonces[0], pts, ads, seq=np.arange(n))
    assert run == [aesgcm.seal(keys[0], aesgcm.seq_nonce(nonces[0], j), pts[j], ads[j]) for j in range(n)]
    got, ok = one.open(nonces[0], run, ads, seq=np.arange(n))
    assert got == pts and ok.all()
    got, ok = one.open(nonces[0], [flip(run[0], 0)] + run[1:], ads, seq=np.arange(n))
    assert got == [bytes(len(pts[0]))] + pts[1:] and ok.tolist() == [0] + [1] * (n - 1)
    torch.cuda.set_device(0)
    d = device.AesGcmDevice(_cuda(kk.copy()))
    rp, ra, tn = device.Ragged(pts), device.Ragged(ads), _cuda(nn.copy())
    ct = d.seal(tn, rp, ra)
    assert ct.cpu().numpy().tobytes() == b"".join(cts)
    pt, ok = d.open(tn, ct, rp, ra)
    assert pt.cpu().numpy()[:-1].tobytes() == b"".join(pts) and bool(ok.all())
    d1 = device.AesGcmDevice(_cuda(kk[0].copy()))
    seq = torch.arange(n, dtype=torch.int64, device="cuda")
    ct = d1.seal(_cuda(nn[0].copy()), rp, ra, seq=seq)
    assert ct.cpu().numpy().tobytes() == b"".join(run)
    pt, ok = d1.open(_cuda(nn[0].copy()), ct, rp, ra, seq=seq)
    assert pt.cpu().numpy()[:-1].tobytes() == b"".join(pts) and bool(ok.all())


# ---- the host pipeline's routes -------------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 items at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices
SPOTS = (0, 99, 100, 199, 200, 255, 256, 299)   # both ends, both sides of the shard boundaries and of the chunk boundary


@pytest.fixture(scope="module")
def pipe(L):
    """this process's own run with the default settings -- one chunk at lo = 0 -- computed once and shared"""
    import aesgcm_worker as aw
    return aw.run(L, 0, N_PIPE)


def _items(flat, lens, extra=0):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [flat[int(off[j]) + extra * j:int(off[j + 1]) + extra * (j + 1)].tobytes() for j in range(len(lens))]


def _check_pipeline_run(o, base):
    """what every configuration asserts about one run of aesgcm_worker.run"""
    import aesgcm_worker as aw
    _, _, _, pts, aads = aw.inputs(N_PIPE)
    lens = [len(x) for x in pts]
    assert lens[0] == lens[255] == lens[256] == 0 and lens[299] == 3 and lens[100] == 26
    for k in base:
        assert o[k].shape == base[k].shape and (np.asarray(o[k]) == base[k]).all(), k
    for name, _ in aw.KEYINGS:
        g = lambda what: o[name + "_" + what]
        assert g("ok").all() and g("pt").tobytes() == b"".join(pts), name
        assert g("ct").size == sum(lens) + 16 * N_PIPE and g("tags").size == 16 * N_PIPE
        ct, ct_noaad, tags = _items(g("ct"), lens, 16), _items(g("ct_noaad"), lens, 16), _items(g("tags"), [0] * N_PIPE, 16)
        for j in SPOTS:
            key, nonce = aw.keying(name, j, N_PIPE)
            assert ct[j] == aesgcm.seal(key, nonce, pts[j], aads[j]) and ct_noaad[j] == aesgcm.seal(key, nonce, pts[j]), (name, j)
            assert tags[j] == aesgcm.seal(key, nonce, b"", aads[j]), (name, j)
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
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "aesgcm_worker.py"), str(device), str(N_PIPE), dst], check=True,
                   env=e, timeout=300)
    _check_pipeline_run(np.load(dst), pipe)
