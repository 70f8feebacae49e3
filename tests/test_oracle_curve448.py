"""The RFC 7748 / RFC 8032 5.2 checker of tests/curve448.py against the reference's own vectors (tests/golden/curve448.json.gz):
the nine Wycheproof keys from their seeds, the 17 valid signatures bit for bit with the empty context (that is how
wycheproof_test.go calls sign/ed448), all 86 verdicts, the six X448 vectors and the iterated ones for 1 and 1000.  CPU only."""
import curve448 as ref
from conftest import load_golden


def test_checker_keys_and_valid_signatures():
    g = load_golden("curve448.json.gz")["wycheproof"]
    keys = {(v["sk"], v["pk"]) for v in g}
    assert len(keys) == 9
    for sk, pk in keys:
        assert ref.public(bytes.fromhex(sk)) == bytes.fromhex(pk)
    valid = [v for v in g if v["valid"]]
    assert len(valid) == 17
    for v in valid:
        sk, pk, msg, sig = (bytes.fromhex(v[k]) for k in ("sk", "pk", "msg", "sig"))
        assert ref.sign(sk + pk, msg, b"") == sig, v["tcId"]


def test_checker_wycheproof_verdicts():
    g = load_golden("curve448.json.gz")["wycheproof"]
    assert len(g) == 86
    for v in g:
        pk, msg, sig = (bytes.fromhex(v[k]) for k in ("pk", "msg", "sig"))
        assert ref.verify(pk, msg, sig) == v["valid"], (v["tcId"], v["comment"])


def test_checker_context_and_rules():
    seed = bytes(range(57))
    pk = ref.public(seed)
    sig = ref.sign(seed + pk, b"msg", b"ctx")
    for rule in ref.RULES:
        assert ref.verify(pk, b"msg", sig, b"ctx", rule)
        assert not ref.verify(pk, b"msg", sig, b"", rule)
    assert not ref.verify(pk, b"msg", sig, bytes(256))
    # S with byte 56 set, S + l: both refused although S + l fits in 56 bytes
    s = int.from_bytes(sig[57:], "little")
    assert not ref.verify(pk, b"msg", sig[:57] + (s + ref.L).to_bytes(57, "little"), b"ctx")
    assert not ref.verify(pk, b"msg", sig[:113] + b"\x01", b"ctx")


def test_checker_x448_vectors():
    g = load_golden("curve448.json.gz")
    assert len(g["x448_kat"]) == 6
    for v in g["x448_kat"]:
        out, ok = ref.x448(bytes.fromhex(v["scalar"]), bytes.fromhex(v["input"]))
        assert ok and out == bytes.fromhex(v["output"])
    assert sorted(v["times"] for v in g["x448_times"]) == [1, 1000]
    want = {v["times"]: bytes.fromhex(v["key"]) for v in g["x448_times"]}
    k = u = (5).to_bytes(56, "little")
    for i in range(1, 1001):
        k, u = ref.x448(k, u)[0], k
        if i in want:
            assert k == want[i], i
    # KeyGen is the ladder from u = 5; the low-order points are flagged and give zeros
    assert ref.x448(bytes(range(56)))[0] == ref.x448(bytes(range(56)), (5).to_bytes(56, "little"))[0]
    for u in (0, 1, ref.P - 1, ref.P, ref.P + 1):
        out, ok = ref.x448(bytes(range(56)), u.to_bytes(56, "little"))
        assert not ok and out == bytes(56)
    out, ok = ref.x448(bytes(range(56)), (2**448 - 1).to_bytes(56, "little"))
    assert ok and out != bytes(56)
