"""Plain-Python checker for Prio3Count / Prio3Sum (draft-irtf-cfrg-vdaf-13 section 7, as the reference's vdaf/prio3 implements it):
big integers mod p = 2^64 - 2^32 + 1 and oracle/k12.py's TurboSHAKE128.  TEST INFRASTRUCTURE ONLY.

It has the operations of the C ABI (shard, prep_init, prep_finish, aggregate, unshard) over single reports, plus `prove` and
`shard_encoded` on a hand-made encoded measurement, so that tests can make cheating clients.  Interpolation is a radix-2 transform with
cached twiddles, so a report at 63 bits costs milliseconds.  All encodings are the reference's MarshalBinary: 8 bytes little-endian per
element, canonical.
"""
import functools

from oracle import k12

P = 2**64 - 2**32 + 1
GEN = 7
COUNT, SUM = 1, 2
SEED = 32
MAX_TRIES = 10


class Prio3Error(Exception):
    pass


def root(l):
    """the root of unity of order 2^l"""
    return pow(GEN, (P - 1) >> l, P)


@functools.lru_cache(maxsize=None)
def _powers(n):
    w, out, x = root(n.bit_length() - 1), [], 1
    for _ in range(n):
        out.append(x)
        x = x * w % P
    return out


def ntt(a, inverse=False):
    """values of the polynomial a (len a power of two) at w^0 .. w^(n-1); inverse: the coefficients from such values"""
    n = len(a)
    if n == 1:
        return list(a)
    pw = _powers(n)
    lg = n.bit_length() - 1
    v = [a[int(format(i, "0%db" % lg)[::-1], 2)] for i in range(n)]
    h = 1
    while h < n:
        step = n // (2 * h)
        for s in range(0, n, 2 * h):
            for i in range(h):
                u, t = v[s + i], v[s + i + h] * pw[i * step] % P
                v[s + i], v[s + i + h] = (u + t) % P, (u - t) % P
        h *= 2
    if inverse:
        ninv = pow(n, P - 2, P)
        v = [v[0]] + v[:0:-1]
        v = [x * ninv % P for x in v]
    return v


def horner(c, x):
    r = 0
    for k in reversed(c):
        r = (r * x + k) % P
    return r


def enc(v):
    return b"".join(int(x).to_bytes(8, "little") for x in v)


def dec(b):
    """None if an element is not canonical"""
    v = [int.from_bytes(b[i:i + 8], "little") for i in range(0, len(b), 8)]
    return None if any(x >= P for x in v) else v


class Task:
    def __init__(self, kind, max_measurement, shares, ctx):
        if kind not in (COUNT, SUM) or not 2 <= shares <= 255 or len(ctx) > 255:
            raise ValueError("task")
        if kind == COUNT and max_measurement != 0 or kind == SUM and not 1 <= max_measurement < 2**63:
            raise ValueError("max_measurement")
        self.kind, self.max, self.shares, self.ctx = kind, max_measurement, shares, bytes(ctx)
        if kind == COUNT:
            self.bits, self.meas_len, self.arity, self.calls, self.eval_out = 0, 1, 2, 1, 1
        else:
            self.bits = max_measurement.bit_length()
            self.meas_len = self.calls = 2 * self.bits
            self.arity, self.eval_out = 1, 2 * self.bits + 1
            self.offset = 2**self.bits - 1 - max_measurement
        self.p = 1
        while self.p < 1 + self.calls:
            self.p *= 2
        self.proof_len = self.arity + 2 * self.p - 1
        self.verifier_len = 2 + self.arity
        self.query_rand_len = 1 + self.eval_out
        self.leader_share_size = 8 * (self.meas_len + self.proof_len)
        self.prep_share_size = 8 * self.verifier_len
        self.rand_size = SEED * shares

    # ---- XofTurboShake128 ----
    def stream(self, usage, seed, binder, nbytes):
        dst = bytes([12, 0]) + self.kind.to_bytes(4, "big") + usage.to_bytes(2, "big") + self.ctx
        return xof(seed, dst, binder, nbytes)

    def vec(self, usage, seed, binder, count):
        """count field elements by rejection sampling, at most MAX_TRIES reads per element"""
        nbytes = 8 * (count + 4)
        while True:
            s = self.stream(usage, seed, binder, nbytes)
            out, tries = [], 0
            for i in range(0, len(s), 8):
                x = int.from_bytes(s[i:i + 8], "little")
                if x < P:
                    out.append(x)
                    tries = 0
                    if len(out) == count:
                        return out
                else:
                    tries += 1
                    if tries == MAX_TRIES:
                        raise Prio3Error("sampler")
            nbytes *= 2

    def helper_meas(self, agg_id, seed):
        return self.vec(1, seed, bytes([agg_id]), self.meas_len)

    def helper_proof(self, agg_id, seed):
        return self.vec(2, seed, bytes([1, agg_id]), self.proof_len)

    # ---- the circuits ----
    def encode(self, m):
        if self.kind == COUNT:
            if m not in (0, 1):
                raise Prio3Error("measurement")
            return [int(m)]
        if not 0 <= m <= self.max:
            raise Prio3Error("measurement")
        return [(m >> i) & 1 for i in range(self.bits)] + [((m + self.offset) >> i) & 1 for i in range(self.bits)]

    def gadget(self, x):
        return x[0] * x[1] % P if self.kind == COUNT else (x[0] * x[0] - x[0]) % P

    def wire_inputs(self, meas):
        """the inputs of gadget call k = 1 .. calls"""
        return [[meas[0], meas[0]]] if self.kind == COUNT else [[x] for x in meas]

    def truncate(self, meas):
        return meas[0] if self.kind == COUNT else sum(meas[i] << i for i in range(self.bits)) % P

    def prove(self, meas, prove_rand):
        """the proof for an ENCODED measurement, valid or not"""
        ins = self.wire_inputs(meas)
        wires = [[prove_rand[a]] + [x[a] for x in ins] + [0] * (self.p - 1 - self.calls) for a in range(self.arity)]
        polys = [ntt(w, inverse=True) for w in wires]
        vals = [ntt(c + [0] * self.p) for c in polys]
        gp = ntt([self.gadget([v[k] for v in vals]) for k in range(2 * self.p)], inverse=True)
        assert gp[-1] == 0
        return [prove_rand[a] for a in range(self.arity)] + gp[:-1]

    def query(self, meas, proof, query_rand):
        seeds, gp = proof[:self.arity], proof[self.arity:]
        folded = ntt([(gp[j] + (gp[j + self.p] if j + self.p < len(gp) else 0)) % P for j in range(self.p)])
        gout = folded[1:1 + self.calls]   # the gadget polynomial at alpha^1 .. alpha^calls
        if self.kind == COUNT:
            v, t = (gout[0] - meas[0]) % P, query_rand[0]
        else:
            b = self.bits
            rc = (self.offset * pow(self.shares, P - 2, P) + sum(meas[i] << i for i in range(b)) - sum(meas[b + i] << i for i in range(b))) % P
            v = sum(o * r for o, r in zip(gout + [rc], query_rand)) % P
            t = query_rand[self.eval_out]
        if pow(t, self.p, P) == 1:
            raise Prio3Error("evaluation point")
        ins = self.wire_inputs(meas)
        checks = []
        for a in range(self.arity):
            w = [seeds[a]] + [x[a] for x in ins] + [0] * (self.p - 1 - self.calls)
            checks.append(horner(ntt(w, inverse=True), t))
        return [v] + checks + [horner(gp, t)]

    def decide(self, verifier):
        return verifier[0] == 0 and self.gadget(verifier[1:1 + self.arity]) == verifier[-1]

    # ---- the operations of the ABI, one report each ----
    def shard_encoded(self, meas, rand):
        """the leader share (bytes) for an encoded measurement; helper j's share is rand[32 (j - 1) : 32 j]"""
        assert len(rand) == self.rand_size
        seeds = [rand[SEED * j:SEED * (j + 1)] for j in range(self.shares)]
        proof = self.prove(meas, self.vec(4, seeds[-1], bytes([1]), self.arity))
        meas = list(meas)
        for j in range(1, self.shares):
            meas = [(a - b) % P for a, b in zip(meas, self.helper_meas(j, seeds[j - 1]))]
            proof = [(a - b) % P for a, b in zip(proof, self.helper_proof(j, seeds[j - 1]))]
        return enc(meas + proof)

    def shard(self, measurement, rand):
        return self.shard_encoded(self.encode(measurement), rand)

    def prep_init(self, agg_id, verify_key, nonce, input_share):
        """(prep share, out share) as bytes"""
        assert agg_id < self.shares
        if agg_id == 0:
            v = dec(input_share)
            if v is None or len(v) != self.meas_len + self.proof_len:
                raise Prio3Error("share")
            meas, proof = v[:self.meas_len], v[self.meas_len:]
        else:
            meas, proof = self.helper_meas(agg_id, input_share), self.helper_proof(agg_id, input_share)
        qr = self.vec(5, verify_key, bytes([1]) + nonce, self.query_rand_len)
        return enc(self.query(meas, proof, qr)), enc([self.truncate(meas)])

    def prep_finish(self, prep_shares):
        """Decide on the summed verifier; prep_shares: the aggregators' prep shares concatenated"""
        v = dec(prep_shares)
        if v is None:
            return False
        n = self.verifier_len
        return self.decide([sum(v[j * n + k] for j in range(self.shares)) % P for k in range(n)])

    def unshard(self, agg_shares, num_measurements):
        if self.kind == SUM and num_measurements * self.max >= P:
            raise Prio3Error("aggregate bound")
        return sum(dec(s)[0] for s in agg_shares) % P


def xof(seed, dst, binder, nbytes):
    return k12.turboshake128(len(dst).to_bytes(2, "little") + dst + bytes([SEED]) + seed + binder, 1, nbytes)


def aggregate(agg_share, out_shares, mask=None):
    s = dec(agg_share)[0]
    for i, o in enumerate(out_shares):
        if mask is None or mask[i]:
            s += dec(o)[0]
    return enc([s % P])
