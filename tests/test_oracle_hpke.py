"""The HPKE DHKEM checker (tests/hpke_dhkem.py) against the 64 RFC 9180 vectors of the reference with kem_id 0x20 / 0x21
(tests/golden/hpke_dhkem.json.gz): derive from every ikm, encap, decap, and for modes 2 and 3 the auth forms in both directions."""
import pytest

import hpke_dhkem as hp
from conftest import hx, load_golden

VECTORS = load_golden("hpke_dhkem.json.gz")


def test_fixture_shape():
    assert len(VECTORS) == 64
    for kem in (0x20, 0x21):
        for mode in range(4):
            assert sum(1 for v in VECTORS if v["kem_id"] == kem and v["mode"] == mode) == 8


@pytest.mark.parametrize("idx", range(64))
def test_vector(idx):
    v = VECTORS[idx]
    k = hp.Kem(v["kem_id"])
    for who in "ERS":
        if "ikm" + who in v:
            assert k.derive_keypair(hx(v["ikm" + who])) == (hx(v["sk%sm" % who]), hx(v["pk%sm" % who])), who
    skR, pkR, enc, ss = hx(v["skRm"]), hx(v["pkRm"]), hx(v["enc"]), hx(v["shared_secret"])
    if v["mode"] in (0, 1):
        assert k.encap(pkR, hx(v["ikmE"])) == (enc, ss)
        assert k.decap(skR, enc) == ss and k.decap(skR, enc, pkR) == ss
    else:
        skS, pkS = hx(v["skSm"]), hx(v["pkSm"])
        assert k.auth_encap(pkR, skS, hx(v["ikmE"])) == (enc, ss)
        assert k.auth_encap(pkR, skS, hx(v["ikmE"]), pkS) == (enc, ss)
        assert k.auth_decap(skR, enc, pkS) == ss and k.auth_decap(skR, enc, pkS, pkR) == ss


@pytest.mark.parametrize("kem", [0x20, 0x21])
def test_low_order_points_fail(kem):
    k = hp.Kem(kem)
    sk, pk = k.derive_keypair(bytes(range(k.N)))
    for pt in hp.low_order_points(kem):
        assert k.encap(pt, bytes(k.N)) is None and k.decap(sk, pt) is None and k.auth_decap(sk, pk, pt) is None
    if kem == 0x20:  # bit 255 is masked before the check
        hi = bytearray(hp.low_order_points(kem)[1])
        hi[31] |= 0x80
        assert k.encap(bytes(hi), bytes(32)) is None
