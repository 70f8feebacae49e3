"""Pins the NIST-curve DLEQ / POPRF checker tests/dleq_nistp.py on the RFC 9497 vectors of the fixture tests/golden/oprf_nistp.json.gz:
the twelve proofs of modes 1 and 2 (six per curve) from their recorded randomness, their verification and tampering, and the mode-2
outputs through tweak -> evaluate -> finalize and through full-evaluate.  CPU only."""
import pytest

import dleq_nistp as dn
import oprf_nistp as on
from conftest import hx, load_golden

G = load_golden("oprf_nistp.json.gz")
CURVES = (256, 384)


def entries(curve):
    return [e for e in G["rfc9497"] if e["identifier"] == on.CURVES[curve].name]


def items(v):
    cols = [v[k].split(",") for k in ("Input", "Blind", "BlindedElement", "EvaluationElement", "Output")]
    assert len({len(c) for c in cols}) == 1 and len(cols[0]) == v["Batch"]
    return [tuple(hx(x) for x in row) for row in zip(*cols)]


def proof_cases(curve):
    """(mode, ctx, k, kA, B, kB, r, proof) of the curve's six fixture proofs; mode 2 proves under the tweaked key with the roles swapped"""
    c = on.CURVES[curve]
    out = []
    for e in entries(curve)[1:]:
        mode, sk = e["mode"], hx(e["skSm"])
        for v in e["vectors"]:
            its = items(v)
            blinded, evaluated = [i[2] for i in its], [i[3] for i in its]
            if mode == 1:
                k, kA, B, kB = sk, hx(e["pkSm"]), blinded, evaluated
            else:
                k, _, kA, ok = dn.poprf_tweak_server(curve, sk, hx(v["Info"]))
                assert ok
                B, kB = evaluated, blinded
            out.append((mode, c.context_string(mode), k, kA, B, kB, hx(v["Proof"]["r"]), hx(v["Proof"]["proof"])))
    return out


CASES = {curve: proof_cases(curve) for curve in CURVES}


def flip(b, bit=0):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


@pytest.mark.parametrize("curve", CURVES)
def test_the_six_proofs_from_their_randomness(curve):
    c = on.CURVES[curve]
    assert [len(x[4]) for x in CASES[curve]] == [1, 1, 2, 1, 1, 2]
    for mode, ctx, k, kA, B, kB, r, proof in CASES[curve]:
        assert len(proof) == 2 * c.Ns
        assert dn.prove(curve, k, kA, B, kB, r, ctx, dn.NO_IDENTITY) == (proof, 1), mode
        assert dn.prove(curve, k, kA, B, kB, r, ctx) == (proof, 1)


@pytest.mark.parametrize("curve", CURVES)
def test_verification_and_tampering(curve):
    c = on.CURVES[curve]
    for mode, ctx, k, kA, B, kB, r, proof in CASES[curve]:
        assert dn.verify(curve, kA, B, kB, proof, ctx, dn.NO_IDENTITY) == 1
        assert dn.verify(curve, kA, B, kB, flip(proof, 3), ctx) == 0                      # c
        assert dn.verify(curve, kA, B, kB, flip(proof, 8 * c.Ns + 5), ctx) == 0           # s
        other = c.encode(c.mul(7, c.G))
        assert dn.verify(curve, kA, B, [other] + kB[1:], proof, ctx) == 0                 # another valid element
        assert dn.verify(curve, kA, [flip(B[0])] + B[1:], kB, proof, ctx) == 0            # the same x, the other y
        assert dn.verify(curve, kA, B, [flip(kB[0], 8 * c.Ne - 1)] + kB[1:], proof, ctx) == 0   # another x, on the curve or not
        assert dn.verify(curve, flip(kA), B, kB, proof, ctx) == 0                         # -kA
        assert dn.verify(curve, other, B, kB, proof, ctx) == 0
        assert dn.verify(curve, kA, B, kB, proof, c.context_string(0)) == 0
        for part in (0, c.Ns):                                                           # c + n, s + n: not canonical
            x = int.from_bytes(proof[part:part + c.Ns], "big") + c.n
            if x < 2 ** (8 * c.Ns):
                assert dn.verify(curve, kA, B, kB, proof[:part] + x.to_bytes(c.Ns, "big") + proof[part + c.Ns:], ctx) == 0


@pytest.mark.parametrize("curve", CURVES)
def test_failure_masks(curve):
    c = on.CURVES[curve]
    mode, ctx, k, kA, B, kB, r, proof = CASES[curve][2]
    zero = (bytes(2 * c.Ns), 0)
    for bad in (bytes(c.Ns), c.n.to_bytes(c.Ns, "big"), (c.n + 1).to_bytes(c.Ns, "big"), b"\xff" * c.Ns):
        assert dn.prove(curve, bad, kA, B, kB, r, ctx) == zero
        assert dn.prove(curve, k, kA, B, kB, bad, ctx) == zero
        assert dn.verify(curve, kA, B, kB, (proof[:c.Ns] + bad) if bad != bytes(c.Ns) else b"\xff" * c.Ns + proof[c.Ns:], ctx) == 0
    assert dn.prove(curve, k, b"\x04" + kA[1:], B, kB, r, ctx) == zero
    assert dn.prove(curve, k, kA, [b"\x02" + b"\xff" * c.Ns] + B[1:], kB, r, ctx) == zero        # x >= p
    assert dn.prove(curve, k, kA, [], [], r, ctx) == zero and dn.verify(curve, kA, [], [], proof, ctx) == 0
    ident = [bytes(c.Ne)]
    p, ok = dn.prove(curve, k, kA, ident, ident, r, ctx)
    assert ok == 1 and dn.verify(curve, kA, ident, ident, p, ctx) == 1                   # zk/dleq accepts the identity ...
    assert dn.prove(curve, k, kA, ident, ident, r, ctx, dn.NO_IDENTITY) == zero          # ... DeserializeElement does not
    assert dn.verify(curve, kA, ident, ident, p, ctx, dn.NO_IDENTITY) == 0


@pytest.mark.parametrize("curve", CURVES)
def test_mode_2_outputs_through_finalize_and_full_evaluate(curve):
    c = on.CURVES[curve]
    e = entries(curve)[2]
    sk, seen = hx(e["skSm"]), 0
    for v in e["vectors"]:
        info = hx(v["Info"])
        t, tinv, tG, ok = dn.poprf_tweak_server(curve, sk, info)
        assert ok and dn.poprf_tweak_client(curve, hx(e["pkSm"]), info) == (tG, 1)
        assert (int.from_bytes(t, "big") * int.from_bytes(tinv, "big")) % c.n == 1 and t == on.poprf_scalar(curve, sk, info)
        for inp, bl, blinded, evaluated, output in items(v):
            assert on.evaluate(curve, tinv, blinded) == (evaluated, 1)
            assert dn.poprf_finalize(curve, inp, info, bl, evaluated) == (output, 1)
            assert dn.poprf_full_evaluate(curve, sk, inp, info) == (output, 1)
            seen += 1
    assert seen == 4


@pytest.mark.parametrize("curve", CURVES)
def test_poprf_failure_masks(curve):
    c = on.CURVES[curve]
    info = b"some info"
    m = dn.info_scalar(c, info)
    fail = (bytes(c.Ns), bytes(c.Ns), bytes(c.Ne), 0)
    assert dn.poprf_tweak_server(curve, c.sc(c.n - m), info) == fail                      # t = 0: ErrInverseZero
    assert dn.poprf_full_evaluate(curve, c.sc(c.n - m), b"x", info) == (bytes(c.Nh), 0)
    minus_mg = c.encode(c.mul(c.n - m, c.G))
    assert dn.poprf_tweak_client(curve, minus_mg, info) == (bytes(c.Ne), 0)               # the tweaked key is the identity
    assert dn.poprf_tweak_client(curve, flip(minus_mg), info)[1] == 1                     # (-m G + m G is not)
    assert dn.poprf_tweak_client(curve, b"\x05" + minus_mg[1:], info) == (bytes(c.Ne), 0)
    assert dn.poprf_tweak_server(curve, c.sc(5), bytes(65536)) == fail and dn.poprf_tweak_client(curve, minus_mg, bytes(65536)) == (bytes(c.Ne), 0)
    assert dn.poprf_tweak_server(curve, c.sc(5), bytes(65535))[3] == 1
    assert dn.poprf_finalize(curve, bytes(65536), info, c.sc(3), minus_mg)[1] == 0 and dn.poprf_finalize(curve, b"", info, c.sc(3), minus_mg)[1] == 1


@pytest.mark.parametrize("curve", CURVES)
def test_generator_multiples_have_a_closed_form(curve):
    """M = (sum of d_j b_j) G where B_j = b_j G: what the GPU tests use to keep long requests cheap"""
    c = on.CURVES[curve]
    mode, ctx, k, kA, _, _, r, _ = CASES[curve][0]
    ks, rs = int.from_bytes(k, "big"), int.from_bytes(r, "big")
    bs = [3, 5, 5, 11]
    B = [c.encode(c.mul(b, c.G)) for b in bs]
    kB = [c.encode(c.mul(b * ks % c.n, c.G)) for b in bs]
    seed = dn.seed_of(c, kA, ctx)
    total = sum(dn.composite_scalar(c, seed, j, B[j], kB[j], ctx) * bs[j] for j in range(len(bs))) % c.n
    closed = dn.proof_from(c, ks, rs, kA, c.mul(total, c.G), ctx)
    assert dn.prove(curve, k, kA, B, kB, r, ctx) == (closed, 1)
    assert dn.verify(curve, kA, B, kB, closed, ctx) == 1
