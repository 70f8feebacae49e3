"""Every exchange form of the Kyber transforms (kyber::Exchange, kyber_dev.h) against the oracle, bit for bit.

circl_hip_kyber_ntt runs the very kyber::ntt / kyber::invntt the ML-KEM kernels use; CIRCL_HIP_NTT_XCH (read at every call) forces the
form: 0 = LDS with barriers, 1 = LDS no-wait, 2 = cross-lane moves (V_PERMLANE32/16_SWAP, DPP row and quad moves), 3 = cross-lane for
L1 <-> L2 only.  The unit polynomials and the index polynomial make every index path of every re-layout distinguishable: a
coefficient that ends up in the wrong (lane, register) slot changes the transform of exactly the polynomials that touch it."""
import os

import numpy as np
import pytest

from circl_amd import hostapi
from oracle import orc

pytestmark = pytest.mark.gpu
Q = 3329
FORMS = {"lds": 0, "lds_nowait": 1, "lanes": 2, "lanes_top": 3}


@pytest.fixture(params=sorted(FORMS), ids=sorted(FORMS))
def form(request):
    old = os.environ.get("CIRCL_HIP_NTT_XCH")
    os.environ["CIRCL_HIP_NTT_XCH"] = str(FORMS[request.param])
    yield request.param
    if old is None:
        del os.environ["CIRCL_HIP_NTT_XCH"]
    else:
        os.environ["CIRCL_HIP_NTT_XCH"] = old


def _want_fwd(p):
    return np.stack([orc.kyber_normalize(orc.kyber_ntt(x)) for x in p])


def _want_inv(p):
    return np.stack([orc.kyber_normalize(orc.kyber_invntt(orc.kyber_normalize(x))) for x in p])


def _index_paths():
    p = np.zeros((257, 256), np.int16)
    p[np.arange(256), np.arange(256)] = 1   # unit polynomial k: coefficient k = 1
    p[256] = np.arange(256)                  # the index polynomial: coefficient k = k
    return p


def test_every_index_path_forward(form):
    p = _index_paths()
    got = hostapi.kyber_ntt(p)
    want = _want_fwd(p)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (form, bad[:8].tolist())


def test_every_index_path_inverse(form):
    p = _index_paths()
    got = hostapi.kyber_ntt(p, inverse=True)
    want = _want_inv(p)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (form, bad[:8].tolist())


def test_random_polynomials_forward(form):
    p = np.random.default_rng(105).integers(-Q + 1, Q, (1 << 12, 256)).astype(np.int16)
    assert (hostapi.kyber_ntt(p) == _want_fwd(p)).all(), form


def test_random_polynomials_inverse(form):
    p = np.random.default_rng(106).integers(-Q + 1, Q, (1 << 12, 256)).astype(np.int16)
    assert (hostapi.kyber_ntt(p, inverse=True) == _want_inv(p)).all(), form


def test_default_form_is_the_ring_phases(monkeypatch):
    """Without the knob the primitive runs the form the big-batch kernels are compiled with (CIRCL_KEM_RING_XCH)."""
    monkeypatch.delenv("CIRCL_HIP_NTT_XCH", raising=False)
    p = _index_paths()
    assert (hostapi.kyber_ntt(p) == _want_fwd(p)).all()
    assert (hostapi.kyber_ntt(p, inverse=True) == _want_inv(p)).all()
