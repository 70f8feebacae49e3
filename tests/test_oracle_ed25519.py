"""The RFC 8032 checker of tests/ed25519.py against the reference's own vectors (tests/golden/ed25519.json.gz): every
sign.input line of the fixture signs and verifies bit for bit, and every Wycheproof verdict matches.  CPU only."""
import ed25519 as ref
from conftest import load_golden


def test_checker_rfc8032_vectors():
    g = load_golden("ed25519.json.gz")["rfc8032"]
    assert len(g) == 352
    for v in g:
        seed, pk, msg, sig = (bytes.fromhex(v[k]) for k in ("seed", "pk", "msg", "sig"))
        assert ref.public(seed) == pk, v["line"]
        assert ref.sign(seed + pk, msg) == sig, v["line"]
        assert ref.verify(pk, msg, sig), v["line"]


def test_checker_wycheproof_verdicts():
    g = load_golden("ed25519.json.gz")["wycheproof"]
    assert len(g) == 145 and sum(v["valid"] for v in g) == 84
    for v in g:
        pk, msg, sig = (bytes.fromhex(v[k]) for k in ("pk", "msg", "sig"))
        assert ref.verify(pk, msg, sig) == v["valid"], (v["tcId"], v["comment"])


def test_checker_hashes_the_stored_public_half():
    # sign/ed25519 hashes sk[32:64] as stored: a foreign public half changes k, hence S, but not R
    seed, other = bytes(range(32)), bytes(range(1, 33))
    sk_good = seed + ref.public(seed)
    sk_bad = seed + ref.public(other)
    a, b = ref.sign(sk_good, b"msg"), ref.sign(sk_bad, b"msg")
    assert a[:32] == b[:32] and a[32:] != b[32:]
    assert not ref.verify(ref.public(seed), b"msg", b)
