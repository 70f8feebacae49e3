"""The CPU checker tests/oprf.py (RFC 9496 / 9380 / 9497 restated) against the fixture tests/golden/oprf_ristretto255.json.gz: the
reference's generator multiples, invalid encodings and scalar lists, and the RFC 9497 vectors of all three modes."""
import pytest

import oprf
from conftest import hx, load_golden

G = load_golden("oprf_ristretto255.json.gz")


def items(v):
    """the (input, blind, blinded, evaluated, output) of every item of a vector (batched ones separate theirs by commas)"""
    cols = [v[k].split(",") for k in ("Input", "Blind", "BlindedElement", "EvaluationElement", "Output")]
    assert len({len(c) for c in cols}) == 1 and len(cols[0]) == v["Batch"]
    return [tuple(hx(x) for x in row) for row in zip(*cols)]


def test_fixture_shape():
    assert [e["mode"] for e in G["rfc9497"]] == [0, 1, 2]
    assert [len(e["vectors"]) for e in G["rfc9497"]] == [2, 3, 3]
    # 2 + 4 + 4 items: the third vector of modes 1 and 2 is a batch of two
    assert [sum(len(items(v)) for v in e["vectors"]) for e in G["rfc9497"]] == [2, 4, 4]
    assert (len(G["multiples"]), len(G["invalid"])) == (16, 29)
    assert [x["enc"][:2] for x in G["invalid"] if x["reference_accepts"]] == ["f3", "ed"]
    assert (len(G["scalars"]["valid"]), len(G["scalars"]["invalid"])) == (3, 5)


def test_constants():
    p, d = oprf.P, oprf.D
    assert d == 37095705934669439343138083508754565189542113879843219016388785533085940283555
    assert oprf.SQRT_M1 == 19681161376707505956807079304988542015446066515923890162744021073123829784752
    assert oprf.ONE_MINUS_D_SQ == 1159843021668779879193775521855586647937357759715417654439879720876111806838
    assert oprf.D_MINUS_ONE_SQ == 40440834346308536858101042469323190826248399146238708352240133220865137265952


def test_generator_multiples():
    p = oprf.IDENTITY
    for k, want in enumerate(G["multiples"]):
        assert oprf.encode(p).hex() == want, k
        assert oprf.encode(oprf.mul(k, oprf.GENERATOR)).hex() == want, k
        assert oprf.encode(oprf.decode(hx(want))).hex() == want, k
        assert oprf.scalar_mult(k.to_bytes(32, "little")) == (hx(want), 1)
        p = oprf.add(p, oprf.GENERATOR)


def test_invalid_encodings_are_rejected():
    for x in G["invalid"]:
        assert oprf.decode(hx(x["enc"])) is None, x
        assert oprf.scalar_mult((1).to_bytes(32, "little"), hx(x["enc"])) == (bytes(32), 0)


def test_scalar_lists():
    for s in G["scalars"]["valid"]:
        assert oprf.decode_scalar(hx(s)) is not None
        assert oprf.scalar_mult(hx(s))[1] == 1
    for s in G["scalars"]["invalid"]:
        assert oprf.decode_scalar(hx(s)) is None
        assert oprf.scalar_mult(hx(s)) == (bytes(32), 0)


def test_scalar_mult_inverse_rules():
    one, zero = (1).to_bytes(32, "little"), bytes(32)
    g = hx(G["multiples"][1])
    assert oprf.scalar_mult(one, None, 1) == (g, 1)
    assert oprf.scalar_mult(zero, None, 1) == (bytes(32), 0)          # an inverse of zero
    assert oprf.scalar_mult(zero, g) == (bytes(32), 1)                # 0 P: the identity, a valid result
    assert oprf.scalar_mult(one, bytes(32)) == (bytes(32), 1)         # the identity is accepted here
    seven = (7).to_bytes(32, "little")
    p, _ = oprf.scalar_mult(seven, g)
    assert p == hx(G["multiples"][7]) and oprf.scalar_mult(seven, p, 1) == (g, 1)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_derive_keypair(mode):
    e = G["rfc9497"][mode]
    sk, pk, ok = oprf.derive_keypair(mode, hx(e["seed"]), hx(e["keyInfo"]))
    assert (sk.hex(), ok) == (e["skSm"], 1)
    if "pkSm" in e:
        assert pk.hex() == e["pkSm"]
    assert oprf.scalar_mult(sk)[0] == pk
    assert e["groupDST"] == (b"HashToGroup-" + oprf.context_string(mode)).hex()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_blinded_elements(mode):
    e = G["rfc9497"][mode]
    for v in e["vectors"]:
        for inp, bl, blinded, _, _ in items(v):
            assert oprf.blind(mode, inp, bl) == (blinded, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_evaluations_and_outputs(mode):
    e = G["rfc9497"][mode]
    sk = hx(e["skSm"])
    for v in e["vectors"]:
        for inp, bl, blinded, evaluated, output in items(v):
            assert oprf.evaluate(sk, blinded) == (evaluated, 1)
            assert oprf.finalize(inp, bl, evaluated) == (output, 1)
            assert oprf.full_evaluate(mode, sk, inp) == (output, 1)


def test_mode_2_evaluations_through_scalar_mult():
    e = G["rfc9497"][2]
    n = 0
    for v in e["vectors"]:
        t = oprf.poprf_scalar(hx(e["skSm"]), hx(v["Info"]))
        for _, _, blinded, evaluated, _ in items(v):
            assert oprf.scalar_mult(t, blinded, 1) == (evaluated, 1)
            n += 1
    assert n == 4


def test_failure_rules():
    e = G["rfc9497"][0]
    sk = hx(e["skSm"])
    inp, bl, blinded, evaluated, _ = items(e["vectors"][0])[0]
    order = oprf.L.to_bytes(32, "little")
    for bad in (bytes(32), order):
        assert oprf.blind(0, inp, bad) == (bytes(32), 0)
        assert oprf.evaluate(bad, blinded) == (bytes(32), 0)
        assert oprf.finalize(inp, bad, evaluated) == (bytes(64), 0)
        assert oprf.full_evaluate(0, bad, inp) == (bytes(64), 0)
    for x in [bytes(32)] + [hx(x["enc"]) for x in G["invalid"]]:
        assert oprf.evaluate(sk, x) == (bytes(32), 0)
        assert oprf.finalize(inp, bl, x) == (bytes(64), 0)
    long_in = bytes(65536)
    assert oprf.blind(0, long_in, bl)[1] == 0 and oprf.finalize(long_in, bl, evaluated)[1] == 0 and oprf.full_evaluate(0, sk, long_in)[1] == 0
    assert oprf.blind(0, long_in[:-1], bl)[1] == 1
