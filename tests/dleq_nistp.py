"""CPU checker for the batch DLEQ proofs of RFC 9497 section 2.2 on P-256 / P-384 (zk/dleq with Params{G, H: the suite's hash, DST}, the
...RFC9497 forms: fixed generator, the base not bound) and for the mode-2 (POPRF) item operations of suites P256-SHA256 / P384-SHA384, on
tests/oprf_nistp.py's Curve and hashlib.  Written from zk/dleq/dleq.go, oprf/client.go and oprf/server.go.  The functions take a curve
(256 or 384) and bytes, return bytes, and follow the C ABI (include/circl_hip.h) operation by operation, `ok` rules included: a failed
request is ok = 0 and an all-zero proof row.  Scalars are big-endian rows of Ns bytes, elements compressed rows of Ne bytes, a proof is
c || s.  It is the yardstick of the GPU tests; tests/test_oracle_dleq_nistp.py pins it on the fixture."""
import oprf_nistp as on

NO_IDENTITY = 1
MAX_BATCH = 0xFFFF


def i2(n):
    return n.to_bytes(2, "big")


def seed_of(c, kA, ctx):
    seed_dst = b"Seed-" + ctx
    return c.hash(i2(c.Ne) + kA + i2(len(seed_dst)) + seed_dst).digest()


def composite_scalar(c, seed, j, b, kb, ctx):
    """d_j of the transcript"""
    return c.hash_to_scalar_int(i2(c.Nh) + seed + i2(j) + i2(c.Ne) + b + i2(c.Ne) + kb + b"Composite", b"HashToScalar-" + ctx)


def _elements(c, rows, flags):
    """the decoded points of a request's rows (None: the identity), or False where one does not decode (or is the identity under
    NO_IDENTITY)"""
    out = []
    for b in rows:
        p = c.decode(bytes(b))
        if p is False or (flags & NO_IDENTITY and p is None):
            return False
        out.append(p)
    return out


def composites(curve, kA, B, kB, ctx, flags=0, with_z=True):
    """(M, Z) as points (Z None unless with_z), or False for a request that fails: 0 or more than 65535 pairs, an element or kA that does
    not decode"""
    c = on.CURVES[curve]
    if not 1 <= len(B) <= MAX_BATCH or len(B) != len(kB) or c.decode(kA) is False:
        return False
    pb, pkb = _elements(c, B, flags), _elements(c, kB, flags)
    if pb is False or pkb is False:
        return False
    seed = seed_of(c, kA, ctx)
    # sum of d_j P_j with the d_j of equal elements added mod n first: one multiplication per DISTINCT element
    sums_m, sums_z = {}, {}
    for j in range(len(B)):
        d = composite_scalar(c, seed, j, bytes(B[j]), bytes(kB[j]), ctx)
        for sums, enc, pt in ((sums_m, bytes(B[j]), pb[j]), (sums_z, bytes(kB[j]), pkb[j])):
            acc = sums.setdefault(enc, [0, pt])
            acc[0] = (acc[0] + d) % c.n
    m, z = None, None
    for d, pt in sums_m.values():
        m = c.add(m, c.mul(d, pt))
    if with_z:
        for d, pt in sums_z.values():
            z = c.add(z, c.mul(d, pt))
    return m, z


def challenge(c, kA, m, z, t2, t3, ctx):
    msg = b"".join(i2(c.Ne) + e for e in (kA, c.encode(m), c.encode(z), c.encode(t2), c.encode(t3))) + b"Challenge"
    return c.hash_to_scalar_int(msg, b"HashToScalar-" + ctx)


def proof_from(c, k, r, kA, m, ctx):
    """the prover's tail on the composite m, k and r as integers"""
    ch = challenge(c, kA, m, c.mul(k, m), c.mul(r, c.G), c.mul(r, m), ctx)
    return c.sc(ch) + c.sc(r - ch * k)


def prove(curve, k, kA, B, kB, r, ctx, flags=0):
    """circl_hip_nistp_dleq_prove, one request: (proof c || s, ok).  k and r must be canonical and not zero (the reference does not test r)."""
    c = on.CURVES[curve]
    ks, rs = on._secret_scalar(c, k), on._secret_scalar(c, r)
    mz = composites(curve, kA, B, kB, ctx, flags, with_z=False) if ks is not None and rs is not None else False
    if mz is False:
        return bytes(2 * c.Ns), 0
    return proof_from(c, ks, rs, kA, mz[0], ctx), 1


def verify(curve, kA, B, kB, proof, ctx, flags=0):
    """circl_hip_nistp_dleq_verify, one request: the verdict"""
    c = on.CURVES[curve]
    ch, s = c.decode_scalar(proof[:c.Ns]), c.decode_scalar(proof[c.Ns:])
    if ch is None or s is None:
        return 0
    mz = composites(curve, kA, B, kB, ctx, flags)
    if mz is False:
        return 0
    m, z = mz
    t2 = c.add(c.mul(s, c.G), c.mul(ch, c.decode(kA)))
    t3 = c.add(c.mul(s, m), c.mul(ch, z))
    return int(challenge(c, kA, m, z, t2, t3, ctx) == ch)


# ---- mode 2 (POPRF) item operations --------------------------------------------------------------------------------------------
def info_scalar(c, info):
    return c.hash_to_scalar_int(b"Info" + i2(len(info)) + info, b"HashToScalar-" + c.context_string(2))


def poprf_tweak_server(curve, sk, info):
    """secretFromInfo: (t, t^-1, t G, ok); ok = 0 for sk zero or >= n, an info over 65535 bytes, t = 0"""
    c = on.CURVES[curve]
    fail = (bytes(c.Ns), bytes(c.Ns), bytes(c.Ne), 0)
    k = on._secret_scalar(c, sk)
    if k is None or len(info) > 0xFFFF:
        return fail
    t = (k + info_scalar(c, info)) % c.n
    if t == 0:
        return fail
    return c.sc(t), c.sc(pow(t, c.n - 2, c.n)), c.encode(c.mul(t, c.G)), 1


def poprf_tweak_client(curve, pkS, info):
    """pointFromInfo: (m G + pkS, ok); ok = 0 where pkS does not decode, the info is over 65535 bytes or the result is the identity"""
    c = on.CURVES[curve]
    p = c.decode(pkS)
    if p is False or len(info) > 0xFFFF:
        return bytes(c.Ne), 0
    out = c.add(c.mul(info_scalar(c, info), c.G), p)
    return (c.encode(out), 1) if out is not None else (bytes(c.Ne), 0)


def _finalize_hash(c, inp, info, element):
    return c.hash(i2(len(inp)) + inp + i2(len(info)) + info + i2(c.Ne) + element + b"Finalize").digest()


def poprf_finalize(curve, inp, info, blind_bytes, evaluated):
    """PartialObliviousClient.Finalize without the proof: (output, ok)"""
    c = on.CURVES[curve]
    k, p = on._secret_scalar(c, blind_bytes), on._element(c, evaluated)
    if k is None or p is None or len(inp) > 0xFFFF or len(info) > 0xFFFF:
        return bytes(c.Nh), 0
    return _finalize_hash(c, inp, info, c.encode(c.mul(pow(k, c.n - 2, c.n), p))), 1


def poprf_full_evaluate(curve, sk, inp, info):
    """PartialObliviousServer.FullEvaluate: (output, ok)"""
    c = on.CURVES[curve]
    t, tinv, _, ok = poprf_tweak_server(curve, sk, info)
    if not ok or len(inp) > 0xFFFF:
        return bytes(c.Nh), 0
    element = c.mul(int.from_bytes(tinv, "big"), c.hash_to_group_point(inp, b"HashToGroup-" + c.context_string(2)))
    return (_finalize_hash(c, inp, info, c.encode(element)), 1) if element is not None else (bytes(c.Nh), 0)
