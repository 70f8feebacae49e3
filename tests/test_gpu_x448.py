"""Batch X448 on the GPU (replaces dh/x448) through the C ABI, against the reference's own vectors (tests/golden/
curve448.json.gz: RFC 7748 known answers and iterated vectors) and the RFC 7748 checker of tests/curve448.py."""
import ctypes as C

import numpy as np
import pytest

import curve448 as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
P = ref.P


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


def _rows(hexes):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), np.uint8).reshape(-1, 56).copy()


def _check(k, u, out, ok, idx):
    for i in idx:
        w_out, w_ok = ref.x448(bytes(k[i]), None if u is None else bytes(u[i]))
        assert bytes(out[i]) == w_out and bool(ok[i]) == w_ok, i


def test_rfc7748_kat(api):
    G = load_golden("curve448.json.gz")["x448_kat"]
    assert len(G) == 6
    out, ok = api.x448(_rows(v["scalar"] for v in G), _rows(v["input"] for v in G))
    assert [bytes(r).hex() for r in out] == [v["output"] for v in G] and ok.all()


def test_rfc7748_times(api):
    # iterate k, u = X448(k, u), k through n = 1 calls: one lane of a wave per call -- latency, not throughput
    want = {v["times"]: v["key"] for v in load_golden("curve448.json.gz")["x448_times"]}
    assert sorted(want) == [1, 1000]
    u = np.zeros((1, 56), np.uint8)
    u[0, 0] = 5
    k = u.copy()
    for t in range(1, 1001):
        r, _ = api.x448(k, u)
        u, k = k, r
        if t in want:
            assert bytes(k[0]).hex() == want[t]


def test_random_pairs_and_keygen_against_the_checker(api):
    n = 4096
    rng = np.random.default_rng(1)
    k = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    u = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    k[0], k[1] = 0, 255   # extreme scalars and points in the mix
    u[2], u[3] = 255, 0
    u[3, 0] = 5
    out, ok = api.x448(k, u)
    _check(k, u, out, ok, range(n))
    k2 = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    pub, okb = api.x448(k2)
    assert okb.all()
    _check(k2, None, pub, okb, range(n))
    five = np.zeros((n, 56), np.uint8)
    five[:, 0] = 5
    assert (api.x448(k2, five)[0] == pub).all()


def test_low_order_points_and_unreduced_aliases(api):
    pts = [0, 1, P - 1, P, P + 1, 2**448 - 1]  # the last reduces to 2^224: an ordinary point
    u = np.frombuffer(b"".join(v.to_bytes(56, "little") for v in pts), np.uint8).reshape(-1, 56).copy()
    k = np.tile(np.arange(56, dtype=np.uint8), (len(pts), 1))
    out, ok = api.x448(k, u)
    assert [int(x) for x in ok] == [0, 0, 0, 0, 0, 1]
    assert not out[:5].any()
    assert bytes(out[5]) == ref.x448(bytes(k[5]), bytes(u[5]))[0] and out[5].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes(api, n):
    rng = np.random.default_rng(n)
    k = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    u = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    out, ok = api.x448(k, u)
    assert out.shape == (n, 56) and ok.shape == (n,)
    _check(k, u, out, ok, sorted({0, n // 2, n - 1}))
    pub, _ = api.x448(k)
    _check(k, None, pub, np.ones(n), sorted({0, n // 2, n - 1}))
    # Diffie-Hellman agreement over the whole batch
    b = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    pb, _ = api.x448(b)
    s1, _ = api.x448(k, pb)
    s2, _ = api.x448(b, pub)
    assert (s1 == s2).all() and s1.any(axis=1).all()


def test_dev_form_on_a_caller_stream(api):
    import torch
    from circl_amd import _native as nat
    rng = np.random.default_rng(3)
    n = 700
    k = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    u = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    u[5] = 0
    dev = torch.device("cuda:0")
    d_k, d_u = torch.from_numpy(k).to(dev), torch.from_numpy(u).to(dev)
    d_out = torch.empty((n, 56), dtype=torch.uint8, device=dev)
    d_pub = torch.empty((n, 56), dtype=torch.uint8, device=dev)
    d_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L_ = nat.lib()
    with torch.cuda.stream(s):
        nat.check(L_.circl_hip_x448_dev(vp(d_k), vp(d_u), vp(d_out), vp(d_ok), n, C.c_void_p(s.cuda_stream)), "x448_dev")
        nat.check(L_.circl_hip_x448_dev(vp(d_k), None, vp(d_pub), None, n, C.c_void_p(s.cuda_stream)), "x448_dev keygen")
    s.synchronize()
    out, ok = api.x448(k, u)
    assert (d_out.cpu().numpy() == out).all() and (d_ok.cpu().numpy() == ok).all() and ok[5] == 0
    assert (d_pub.cpu().numpy() == api.x448(k)[0]).all()
    _check(k, u, out, ok, [0, 5, 699])


def test_every_device_and_all_devices(api):
    rng = np.random.default_rng(4)
    n = 5000
    k = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    u = rng.integers(0, 256, (n, 56), dtype=np.uint8)
    base, base_ok = api.x448(k, u, device=0)
    _check(k, u, base, base_ok, [0, 1, n - 1])
    for d in list(range(1, api.device_count())) + [-1]:
        out, ok = api.x448(k, u, device=d)
        assert (out == base).all() and (ok == base_ok).all(), d
        assert (api.x448(k, device=d)[0] == api.x448(k, device=0)[0]).all(), d
