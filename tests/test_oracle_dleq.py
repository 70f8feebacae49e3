"""Pins the DLEQ / POPRF checker tests/dleq.py on the RFC 9497 vectors of the fixture: the six proofs of modes 1 and 2 from their
recorded randomness, their verification, and the four mode-2 outputs."""
import dleq
import oprf
from conftest import hx, load_golden
from test_oracle_oprf import items

G = load_golden("oprf_ristretto255.json.gz")
L = oprf.L


def proof_cases():
    """(mode, ctx, k, kA, B, kB, r, proof) of the six fixture proofs; mode 2 proves under the tweaked key with the roles swapped"""
    out = []
    for e in G["rfc9497"][1:]:
        mode, sk = e["mode"], hx(e["skSm"])
        for v in e["vectors"]:
            its = items(v)
            blinded, evaluated = [i[2] for i in its], [i[3] for i in its]
            if mode == 1:
                k, kA, B, kB = sk, hx(e["pkSm"]), blinded, evaluated
            else:
                k, _, kA, ok = dleq.poprf_tweak_server(sk, hx(v["Info"]))
                assert ok
                B, kB = evaluated, blinded
            out.append((mode, oprf.context_string(mode), k, kA, B, kB, hx(v["Proof"]["r"]), hx(v["Proof"]["proof"])))
    return out


CASES = proof_cases()


def flip(b, bit=0):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def test_the_six_proofs_from_their_randomness():
    assert [len(c[4]) for c in CASES] == [1, 1, 2, 1, 1, 2]
    for mode, ctx, k, kA, B, kB, r, proof in CASES:
        assert dleq.prove(k, kA, B, kB, r, ctx, dleq.NO_IDENTITY) == (proof, 1), mode
        assert dleq.prove(k, kA, B, kB, r, ctx) == (proof, 1)


def test_verification_and_tampering():
    for mode, ctx, k, kA, B, kB, r, proof in CASES:
        assert dleq.verify(kA, B, kB, proof, ctx, dleq.NO_IDENTITY) == 1
        assert dleq.verify(kA, B, kB, flip(proof, 3), ctx) == 0                  # c
        assert dleq.verify(kA, B, kB, flip(proof, 256 + 5), ctx) == 0            # s
        other = oprf.encode(oprf.mul(7, oprf.GENERATOR))
        assert dleq.verify(kA, B, [other] + kB[1:], proof, ctx) == 0             # another valid element
        assert dleq.verify(kA, B, [flip(kB[0])] + kB[1:], proof, ctx) == 0       # s odd: does not decode
        assert dleq.verify(kA, B, kB, proof, oprf.context_string(0)) == 0
        for part in (0, 32):                                                    # c + L, s + L: not canonical
            x = int.from_bytes(proof[part:part + 32], "little") + L
            assert dleq.verify(kA, B, kB, proof[:part] + x.to_bytes(32, "little") + proof[part + 32:], ctx) == 0


def test_failure_masks():
    mode, ctx, k, kA, B, kB, r, proof = CASES[2]
    le = lambda x: x.to_bytes(32, "little")
    for bad in (bytes(32), le(L), le(L + 1), b"\xff" * 32):
        assert dleq.prove(bad, kA, B, kB, r, ctx) == (bytes(64), 0)
        assert dleq.prove(k, kA, B, kB, bad, ctx) == (bytes(64), 0)
    assert dleq.prove(k, flip(kA), B, kB, r, ctx) == (bytes(64), 0)
    assert dleq.prove(k, kA, [], [], r, ctx) == (bytes(64), 0) and dleq.verify(kA, [], [], proof, ctx) == 0
    ident = [bytes(32)]
    p, ok = dleq.prove(k, kA, ident, ident, r, ctx)
    assert ok == 1 and dleq.verify(kA, ident, ident, p, ctx) == 1               # zk/dleq accepts the identity ...
    assert dleq.prove(k, kA, ident, ident, r, ctx, dleq.NO_IDENTITY) == (bytes(64), 0)      # ... DeserializeElement does not
    assert dleq.verify(kA, ident, ident, p, ctx, dleq.NO_IDENTITY) == 0


def test_mode_2_outputs_through_finalize_and_full_evaluate():
    e = G["rfc9497"][2]
    sk, seen = hx(e["skSm"]), 0
    for v in e["vectors"]:
        info = hx(v["Info"])
        t, tinv, tG, ok = dleq.poprf_tweak_server(sk, info)
        assert ok and dleq.poprf_tweak_client(hx(e["pkSm"]), info) == (tG, 1)
        assert (int.from_bytes(t, "little") * int.from_bytes(tinv, "little")) % L == 1 and t == oprf.poprf_scalar(sk, info)
        for inp, bl, blinded, evaluated, output in items(v):
            assert oprf.evaluate(tinv, blinded) == (evaluated, 1)
            assert dleq.poprf_finalize(inp, info, bl, evaluated) == (output, 1)
            assert dleq.poprf_full_evaluate(sk, inp, info) == (output, 1)
            seen += 1
    assert seen == 4


def test_poprf_failure_masks():
    info = b"some info"
    m = dleq.info_scalar(info)
    le = lambda x: x.to_bytes(32, "little")
    assert dleq.poprf_tweak_server(le(L - m), info) == (bytes(32), bytes(32), bytes(32), 0)          # t = 0: ErrInverseZero
    assert dleq.poprf_full_evaluate(le(L - m), b"x", info) == (bytes(64), 0)
    minus_mg = oprf.encode(oprf.mul(L - m, oprf.GENERATOR))
    assert dleq.poprf_tweak_client(minus_mg, info) == (bytes(32), 0)                                 # the tweaked key is the identity
    assert dleq.poprf_tweak_client(flip(minus_mg), info) == (bytes(32), 0)
    assert dleq.poprf_tweak_server(le(5), bytes(65536))[3] == 0 and dleq.poprf_tweak_client(minus_mg, bytes(65536)) == (bytes(32), 0)
    assert dleq.poprf_tweak_server(le(5), bytes(65535))[3] == 1


def test_65535_copies_of_one_pair_have_a_closed_form():
    """M = (sum of d_j mod L) B when every pair is the same: the full-length batch costs hashes only"""
    mode, ctx, k, kA, B, kB, r, _ = CASES[0]
    n = dleq.MAX_BATCH
    seed = dleq.seed_of(kA, ctx)
    total = sum(dleq.composite_scalar(seed, j, B[0], kB[0], ctx) for j in range(n)) % L
    pb, ks, rs = oprf.decode(B[0]), int.from_bytes(k, "little"), int.from_bytes(r, "little")
    m = oprf.mul(total, pb)
    c = dleq.challenge(kA, m, oprf.mul(ks, m), oprf.mul(rs, oprf.GENERATOR), oprf.mul(rs, m), ctx)
    closed = c.to_bytes(32, "little") + ((rs - c * ks) % L).to_bytes(32, "little")
    assert dleq.prove(k, kA, B * n, kB * n, r, ctx) == (closed, 1)
    assert dleq.verify(kA, B * n, kB * n, closed, ctx) == 1
    # the verifier's side, in closed form: Z = total kB
    z = oprf.mul(total, oprf.decode(kB[0]))
    s = int.from_bytes(closed[32:], "little")
    t2 = oprf.add(oprf.mul(s, oprf.GENERATOR), oprf.mul(c, oprf.decode(kA)))
    t3 = oprf.add(oprf.mul(s, m), oprf.mul(c, z))
    assert dleq.challenge(kA, m, z, t2, t3, ctx) == c
    assert dleq.prove(k, kA, B * (n + 1), kB * (n + 1), r, ctx) == (bytes(64), 0)
