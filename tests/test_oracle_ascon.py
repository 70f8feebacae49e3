"""The checker tests/ascon.py against every vector of tests/golden/ascon.json.gz (the reference's cipher/ascon/testdata): Seal, Open,
and Open of one flipped bit in each of ct, tag, aad, nonce and key.  CPU only."""
import pytest

import ascon
from conftest import hx, load_golden

G = load_golden("ascon.json.gz")


def flip(b, bit=0):
    b = bytearray(b)
    b[bit // 8 % len(b)] ^= 1 << bit % 8
    return bytes(b)


def vectors(name):
    """(key, nonce, [(pt, ad, ct)])"""
    e = G[name]
    return hx(e["Key"]), hx(e["Nonce"]), [(hx(v["PT"]), hx(v["AD"]), hx(v["CT"])) for v in e["vectors"]]


def test_the_fixture_is_whole():
    assert sorted(G) == sorted(ascon.MODES)
    for name, mode in ascon.MODES.items():
        key, nonce, vs = vectors(name)
        assert len(key) == ascon.key_size(mode) and len(nonce) == 16 and len(vs) == 1089
        assert {(len(pt), len(ad)) for pt, ad, _ in vs} == {(p, a) for p in range(33) for a in range(33)}
        assert all(len(ct) == len(pt) + 16 for pt, _, ct in vs)


@pytest.mark.parametrize("name", sorted(ascon.MODES))
def test_seal_and_open_on_every_vector(name):
    mode = ascon.MODES[name]
    key, nonce, vs = vectors(name)
    for pt, ad, ct in vs:
        assert ascon.seal(mode, key, nonce, pt, ad) == ct
        assert ascon.open(mode, key, nonce, ct, ad) == pt


@pytest.mark.parametrize("name", sorted(ascon.MODES))
def test_open_refuses_one_flipped_bit(name):
    mode = ascon.MODES[name]
    key, nonce, vs = vectors(name)
    for j, (pt, ad, ct) in enumerate(vs):
        if pt:
            assert ascon.open(mode, key, nonce, flip(ct[:-16], j) + ct[-16:], ad) is None
        assert ascon.open(mode, key, nonce, ct[:-16] + flip(ct[-16:], j), ad) is None
        if ad:
            assert ascon.open(mode, key, nonce, ct, flip(ad, j)) is None
        assert ascon.open(mode, flip(key, j), nonce, ct, ad) is None
        assert ascon.open(mode, key, flip(nonce, j), ct, ad) is None
    assert ascon.open(mode, key, nonce, vs[0][2][:15]) is None
