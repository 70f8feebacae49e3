"""Batch FrodoKEM-640-SHAKE on the GPU (replaces kem/frodo/frodo640shake) through the C ABI: the reference's KAT pin
(tests/golden/frodo640shake.json, kem/frodo/kat_test.go) with nothing in between, and bit-exact against the checker of
tests/frodo.py for the batch shapes, implicit rejection, keys taken as stored, the _dev forms, the devices and the profiling ids.
The checker's 130 reference items are computed once per session and shared."""
import ctypes as C

import numpy as np
import pytest

import frodo as ref
from frodo import golden, kat_seeds, kat_transcript

pytestmark = pytest.mark.gpu
NMAX = 130


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


def _rows(items, cols):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, cols).copy()


@pytest.fixture(scope="module")
def items():
    """130 items from the checker: seeds of all zeros and all 0xFF in front"""
    rng = np.random.default_rng(640)
    seeds = [bytes(48), b"\xff" * 48] + [rng.bytes(48) for _ in range(NMAX - 2)]
    mus = [bytes(16), b"\xff" * 16] + [rng.bytes(16) for _ in range(NMAX - 2)]
    pk, sk, ct, ss = [], [], [], []
    for s, m in zip(seeds, mus):
        p, k = ref.keygen(s)
        c, x = ref.encaps(p, m)
        pk.append(p), sk.append(k), ct.append(c), ss.append(x)
    return dict(seed=_rows(seeds, 48), mu=_rows(mus, 16), pk=_rows(pk, ref.PK_BYTES), sk=_rows(sk, ref.SK_BYTES), ct=_rows(ct, ref.CT_BYTES),
                ss=_rows(ss, 16))


def test_kat_transcript(api):
    g = golden()
    seeds = kat_seeds(g["kat_count"])
    pk, sk = api.frodo640shake_keygen(_rows([k for _, k, _ in seeds], 48))
    ct, ss = api.frodo640shake_encaps(pk, _rows([e for _, _, e in seeds], 16))
    ss2 = api.frodo640shake_decaps(sk, ct)
    assert (ss2 == ss).all()
    entries = [(seeds[i][0], pk[i].tobytes(), sk[i].tobytes(), ct[i].tobytes(), ss[i].tobytes()) for i in range(len(seeds))]
    assert kat_transcript(g["name"], entries) == g["kat_sha256"]


@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_batch_shapes(api, items, n):
    pk, sk = api.frodo640shake_keygen(items["seed"][:n])
    assert (pk == items["pk"][:n]).all() and (sk == items["sk"][:n]).all()
    ct, ss = api.frodo640shake_encaps(items["pk"][:n], items["mu"][:n])
    assert (ct == items["ct"][:n]).all() and (ss == items["ss"][:n]).all()
    assert (api.frodo640shake_decaps(items["sk"][:n], items["ct"][:n]) == items["ss"][:n]).all()


def test_implicit_rejection(api, items):
    n = 65
    ct = items["ct"][:n].copy()
    where = [None, 0, 9599, 9600, 9719]  # untouched, then the ends of pack(B') and of pack(C)
    for i in range(n):
        b = where[i % 5]
        if b is not None:
            ct[i, b] ^= 1 << (i % 8)
    ss = api.frodo640shake_decaps(items["sk"][:n], ct)
    for i in range(n):
        want = ref.decaps(items["sk"][i].tobytes(), ct[i].tobytes())
        assert ss[i].tobytes() == want, i
        if where[i % 5] is None:
            assert want == items["ss"][i].tobytes()
        else:
            assert want == ref.shake128(ct[i].tobytes() + items["sk"][i, :16].tobytes(), 16) and want != items["ss"][i].tobytes()


def test_keys_taken_as_stored(api, items):
    sk = items["sk"][:3].copy()
    ct = items["ct"][:3].copy()
    s0 = 16 + ref.PK_BYTES
    sk[0, -16:] ^= 0xA5                                        # another hpk: used as it is, so the re-encryption differs
    sk[1, :16] ^= 0x3C                                         # another s ...
    ct[1, 100] ^= 2                                            # ... which shows in the rejection key
    odd = np.array([0x8000, 0xFFFF, 0x7FFF] * 40, "<u2")        # S^T words that are no samples
    sk[2, s0:s0 + 240] = np.frombuffer(odd.tobytes(), np.uint8)
    sk[2, s0 + 2 * 5000: s0 + 2 * 5000 + 240] = np.frombuffer(odd.tobytes(), np.uint8)
    ss = api.frodo640shake_decaps(sk, ct)
    for i in range(3):
        assert ss[i].tobytes() == ref.decaps(sk[i].tobytes(), ct[i].tobytes()), i
    assert ss[0].tobytes() != items["ss"][0].tobytes()
    # a public key whose packed B is all ones
    pk = items["pk"][:1].copy()
    pk[0, 16:] = 0xFF
    ctx, ssx = api.frodo640shake_encaps(pk, items["mu"][:1])
    w_ct, w_ss = ref.encaps(pk[0].tobytes(), items["mu"][0].tobytes())
    assert ctx[0].tobytes() == w_ct and ssx[0].tobytes() == w_ss


def test_dev_forms(items):
    import torch
    from circl_amd import _native as nat
    n = 65
    L = nat.lib()
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    vp = lambda x: C.c_void_p(x.data_ptr())    # noqa: E731
    d_seed, d_mu = t(items["seed"][:n]), t(items["mu"][:n])
    d_pk = torch.zeros((n, ref.PK_BYTES), dtype=torch.uint8, device=dev)
    d_sk = torch.zeros((n, ref.SK_BYTES), dtype=torch.uint8, device=dev)
    d_ct = torch.zeros((n, ref.CT_BYTES), dtype=torch.uint8, device=dev)
    d_ss = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    d_ss2 = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    wsb = L.circl_hip_frodo640shake_workspace_size(n)
    assert wsb >= n * 20608 and L.circl_hip_frodo640shake_workspace_size(n + 1) >= wsb and L.circl_hip_frodo640shake_workspace_size(0) == 0
    d_ws = torch.full((wsb + 16,), 0x77, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for ws_ptr, ws_len in ((d_ws.data_ptr(), wsb - 256), (d_ws.data_ptr() + 4, wsb)):  # short, misaligned
            ws_ptr = C.c_void_p(ws_ptr)
            assert L.circl_hip_frodo640shake_keygen_dev(vp(d_seed), vp(d_pk), vp(d_sk), n, ws_ptr, ws_len, st) == nat.EWORKSPACE
            assert L.circl_hip_frodo640shake_encaps_dev(vp(d_pk), vp(d_mu), vp(d_ct), vp(d_ss), n, ws_ptr, ws_len, st) == nat.EWORKSPACE
            assert L.circl_hip_frodo640shake_decaps_dev(vp(d_sk), vp(d_ct), vp(d_ss2), n, ws_ptr, ws_len, st) == nat.EWORKSPACE
        assert L.circl_hip_frodo640shake_keygen_dev(None, vp(d_pk), vp(d_sk), n, vp(d_ws), wsb, st) == nat.EPARAM
        assert L.circl_hip_frodo640shake_encaps_dev(vp(d_pk), vp(d_mu), None, vp(d_ss), n, vp(d_ws), wsb, st) == nat.EPARAM
        assert L.circl_hip_frodo640shake_decaps_dev(vp(d_sk), vp(d_ct), vp(d_ss2), n, None, wsb, st) == nat.EPARAM
        assert L.circl_hip_frodo640shake_keygen_dev(None, None, None, 0, None, 0, st) == nat.OK
        assert L.circl_hip_frodo640shake_encaps_dev(None, None, None, None, 0, None, 0, st) == nat.OK
        assert L.circl_hip_frodo640shake_decaps_dev(None, None, None, 0, None, 0, st) == nat.OK
        zeros = []
        nat.check(L.circl_hip_frodo640shake_keygen_dev(vp(d_seed), vp(d_pk), vp(d_sk), n, vp(d_ws), wsb, st), "keygen_dev")
        zeros.append(d_ws[:wsb].clone())
        nat.check(L.circl_hip_frodo640shake_encaps_dev(vp(d_pk), vp(d_mu), vp(d_ct), vp(d_ss), n, vp(d_ws), wsb, st), "encaps_dev")
        zeros.append(d_ws[:wsb].clone())
        nat.check(L.circl_hip_frodo640shake_decaps_dev(vp(d_sk), vp(d_ct), vp(d_ss2), n, vp(d_ws), wsb, st), "decaps_dev")
        zeros.append(d_ws[:wsb].clone())
    s.synchronize()
    for z in zeros:
        assert int(z.max()) == 0          # the workspace is secret and reads zero behind every call
    assert int(d_ws[wsb:].min()) == 0x77    # nothing behind it was touched
    assert (d_pk.cpu().numpy() == items["pk"][:n]).all() and (d_sk.cpu().numpy() == items["sk"][:n]).all()
    assert (d_ct.cpu().numpy() == items["ct"][:n]).all() and (d_ss.cpu().numpy() == items["ss"][:n]).all()
    assert (d_ss2.cpu().numpy() == items["ss"][:n]).all()
    # rows at odd byte offsets: the _dev forms promise no alignment
    flat = torch.zeros(n * ref.CT_BYTES + 8, dtype=torch.uint8, device=dev)
    flat_sk = torch.zeros(n * ref.SK_BYTES + 8, dtype=torch.uint8, device=dev)
    flat[3:3 + n * ref.CT_BYTES] = d_ct.reshape(-1)
    flat_sk[1:1 + n * ref.SK_BYTES] = d_sk.reshape(-1)
    d_ss2.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        nat.check(L.circl_hip_frodo640shake_decaps_dev(C.c_void_p(flat_sk.data_ptr() + 1), C.c_void_p(flat.data_ptr() + 3), vp(d_ss2), n, vp(d_ws), wsb, st),
                  "decaps_dev, odd offsets")
    s.synchronize()
    assert (d_ss2.cpu().numpy() == items["ss"][:n]).all()


def test_devices_agree(api, items):
    outs = []
    for device in [-1] + list(range(api.device_count())):
        pk, sk = api.frodo640shake_keygen(items["seed"], device=device)
        ct, ss = api.frodo640shake_encaps(items["pk"], items["mu"], device=device)
        ss2 = api.frodo640shake_decaps(items["sk"], items["ct"], device=device)
        outs.append((pk, sk, ct, ss, ss2))
    want = (items["pk"], items["sk"], items["ct"], items["ss"], items["ss"])
    for o in outs:
        for got, w in zip(o, want):
            assert (got == w).all()


def test_profiling_ids(api, items):
    from circl_amd import device as dv
    assert (dv.KERNELS["frodo_keygen"], dv.KERNELS["frodo_encaps"], dv.KERNELS["frodo_decaps"]) == (20, 21, 22)
    dv.profile_enable(True)
    try:
        for k in ("frodo_keygen", "frodo_encaps", "frodo_decaps"):
            dv.profile_read(k)
        api.frodo640shake_keygen(items["seed"][:3])
        api.frodo640shake_encaps(items["pk"][:3], items["mu"][:3])
        api.frodo640shake_decaps(items["sk"][:3], items["ct"][:3])
        for k in ("frodo_keygen", "frodo_encaps", "frodo_decaps"):
            ms, cnt = dv.profile_read(k)
            assert ms > 0 and cnt >= 1, k
    finally:
        dv.profile_enable(False)
