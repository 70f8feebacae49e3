"""CPU checker for the batch DLEQ proofs of RFC 9497 section 2.2 on ristretto255 (zk/dleq, the ...RFC9497 forms: fixed generator, the
base not bound) and for the mode-2 (POPRF) item operations, on tests/oprf.py.  The functions take and return bytes and follow the C ABI
(include/circl_hip.h) operation by operation, `ok` rules included: a failed request is ok = 0 and an all-zero proof row.  It is the
yardstick of the GPU tests; tests/test_oracle_dleq.py pins it on the fixture."""
import hashlib

import oprf
from oprf import L, ZERO32, ZERO64

NO_IDENTITY = 1
MAX_BATCH = 0xFFFF
ZERO_PROOF = bytes(64)


def i2(n):
    return n.to_bytes(2, "big")


def seed_of(kA, ctx):
    seed_dst = b"Seed-" + ctx
    return hashlib.sha512(i2(32) + kA + i2(len(seed_dst)) + seed_dst).digest()


def composite_scalar(seed, j, b, kb, ctx):
    """d_j of the transcript"""
    return oprf.hash_to_scalar_int(i2(64) + seed + i2(j) + i2(32) + b + i2(32) + kb + b"Composite", b"HashToScalar-" + ctx)


def _elements(rows, flags):
    """the decoded points of a request's rows, or None where one does not decode (or is the identity under NO_IDENTITY)"""
    out = []
    for b in rows:
        p = oprf.decode(bytes(b))
        if p is None or (flags & NO_IDENTITY and bytes(b) == ZERO32):
            return None
        out.append(p)
    return out


def composites(kA, B, kB, ctx, flags=0, with_z=True):
    """(M, Z) as points (Z None unless with_z), or None for a request that fails: 0 or more than 65535 pairs, an element or kA that does
    not decode"""
    if not 1 <= len(B) <= MAX_BATCH or len(B) != len(kB) or oprf.decode(kA) is None:
        return None
    pb, pkb = _elements(B, flags), _elements(kB, flags)
    if pb is None or pkb is None:
        return None
    seed = seed_of(kA, ctx)
    # sum of d_j P_j with the d_j of equal elements added mod L first: one multiplication per DISTINCT element
    sums_m, sums_z = {}, {}
    for j in range(len(B)):
        d = composite_scalar(seed, j, bytes(B[j]), bytes(kB[j]), ctx)
        for sums, enc, pt in ((sums_m, bytes(B[j]), pb[j]), (sums_z, bytes(kB[j]), pkb[j])):
            acc = sums.setdefault(enc, [0, pt])
            acc[0] = (acc[0] + d) % L
    m, z = oprf.IDENTITY, oprf.IDENTITY
    for d, pt in sums_m.values():
        m = oprf.add(m, oprf.mul(d, pt))
    if with_z:
        for d, pt in sums_z.values():
            z = oprf.add(z, oprf.mul(d, pt))
    return m, (z if with_z else None)


def challenge(kA, m, z, t2, t3, ctx):
    msg = b"".join(i2(32) + e for e in (kA, oprf.encode(m), oprf.encode(z), oprf.encode(t2), oprf.encode(t3))) + b"Challenge"
    return oprf.hash_to_scalar_int(msg, b"HashToScalar-" + ctx)


def prove(k, kA, B, kB, r, ctx, flags=0):
    """circl_hip_dleq_prove, one request: (proof c || s, ok).  k and r must be canonical and not zero (the reference does not test r)."""
    ks, rs = oprf._secret_scalar(k), oprf._secret_scalar(r)
    if ks is None or rs is None:
        return ZERO_PROOF, 0
    mz = composites(kA, B, kB, ctx, flags, with_z=False)
    if mz is None:
        return ZERO_PROOF, 0
    m = mz[0]
    c = challenge(kA, m, oprf.mul(ks, m), oprf.mul(rs, oprf.GENERATOR), oprf.mul(rs, m), ctx)
    s = (rs - c * ks) % L
    return c.to_bytes(32, "little") + s.to_bytes(32, "little"), 1


def verify(kA, B, kB, proof, ctx, flags=0):
    """circl_hip_dleq_verify, one request: the verdict"""
    c, s = oprf.decode_scalar(proof[:32]), oprf.decode_scalar(proof[32:])
    if c is None or s is None:
        return 0
    mz = composites(kA, B, kB, ctx, flags)
    if mz is None:
        return 0
    m, z = mz
    t2 = oprf.add(oprf.mul(s, oprf.GENERATOR), oprf.mul(c, oprf.decode(kA)))
    t3 = oprf.add(oprf.mul(s, m), oprf.mul(c, z))
    return int(challenge(kA, m, z, t2, t3, ctx) == c)


# ---- mode 2 (POPRF) item operations --------------------------------------------------------------------------------------------
CTX2 = oprf.context_string(2)


def info_scalar(info):
    return oprf.hash_to_scalar_int(b"Info" + i2(len(info)) + info, b"HashToScalar-" + CTX2)


def poprf_tweak_server(sk, info):
    """secretFromInfo: (t, t^-1, t G, ok); ok = 0 for sk zero or >= L, an info over 65535 bytes, t = 0"""
    k = oprf._secret_scalar(sk)
    if k is None or len(info) > 0xFFFF:
        return ZERO32, ZERO32, ZERO32, 0
    t = (k + info_scalar(info)) % L
    if t == 0:
        return ZERO32, ZERO32, ZERO32, 0
    return t.to_bytes(32, "little"), pow(t, L - 2, L).to_bytes(32, "little"), oprf.encode(oprf.mul(t, oprf.GENERATOR)), 1


def poprf_tweak_client(pkS, info):
    """pointFromInfo: (m G + pkS, ok); ok = 0 where pkS does not decode, the info is over 65535 bytes or the result is the identity"""
    p = oprf.decode(pkS)
    if p is None or len(info) > 0xFFFF:
        return ZERO32, 0
    out = oprf.encode(oprf.add(oprf.mul(info_scalar(info), oprf.GENERATOR), p))
    return (out, 1) if out != ZERO32 else (ZERO32, 0)


def _finalize_hash(inp, info, element):
    return hashlib.sha512(i2(len(inp)) + inp + i2(len(info)) + info + i2(32) + element + b"Finalize").digest()


def poprf_finalize(inp, info, blind_bytes, evaluated):
    """PartialObliviousClient.Finalize without the proof: (output, ok)"""
    k, p = oprf._secret_scalar(blind_bytes), oprf._element(evaluated)
    if k is None or p is None or len(inp) > 0xFFFF or len(info) > 0xFFFF:
        return ZERO64, 0
    return _finalize_hash(inp, info, oprf.encode(oprf.mul(pow(k, L - 2, L), p))), 1


def poprf_full_evaluate(sk, inp, info):
    """PartialObliviousServer.FullEvaluate: (output, ok)"""
    t, tinv, _, ok = poprf_tweak_server(sk, info)
    if not ok or len(inp) > 0xFFFF:
        return ZERO64, 0
    element = oprf.encode(oprf.mul(int.from_bytes(tinv, "little"), oprf.hash_to_group_point(inp, b"HashToGroup-" + CTX2)))
    return (_finalize_hash(inp, info, element), 1) if element != ZERO32 else (ZERO64, 0)
