"""CPU checker for the NIST P-256 / P-384 groups (SEC 1 compressed points), their hash-to-curve / hash-to-scalar (RFC 9380: expand_message_xmd,
hash_to_field, simplified SWU for p = 3 mod 4) and the proof-free part of OPRF (RFC 9497, suites P256-SHA256 and P384-SHA384): big integers
and hashlib, written from the RFCs and SEC 1.  The functions of the second half take a curve and bytes, return bytes, and follow the C ABI
(include/circl_hip.h) operation by operation, `ok` rules included: a failed item is ok = 0 and zero rows.  It is the yardstick of the GPU
tests; tests/test_oracle_oprf_nistp.py checks it against the fixture and against libcrypto."""
import hashlib


class Curve:
    def __init__(self, bits, p, b, n, gx, gy, z, c2, hash_name, ell, name):
        self.bits, self.p, self.b, self.n, self.z, self.ell, self.name = bits, p, b, n, z % p, ell, name
        self.a = p - 3
        self.G = (gx, gy)
        self.hash = getattr(hashlib, hash_name)
        self.Ns = bits // 8                 # a scalar, a field element
        self.Ne = self.Ns + 1               # a compressed point
        self.Nh = self.hash().digest_size   # an OPRF output
        self.c1 = (p - 3) // 4
        self.c2 = c2                        # RFC 9380 F.2.1.2: sqrt(-Z^3), the root that 8.2 / 8.3 list
        assert p % 4 == 3 and self.c2 * self.c2 % p == -self.z ** 3 % p and self.on_curve(self.G) and self.mul_affine(n, self.G) is None

    def on_curve(self, pt):
        x, y = pt
        return (y * y - (x * x * x + self.a * x + self.b)) % self.p == 0

    # ---- affine points; None is the identity ------------------------------------------------------------------------------
    def add(self, P, Q):
        p = self.p
        if P is None:
            return Q
        if Q is None:
            return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = (3 * x1 * x1 + self.a) * pow(2 * y1, p - 2, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, p - 2, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return (x3, (lam * (x1 - x3) - y1) % p)

    def mul_affine(self, k, P):
        """double-and-add on the affine law above: slow, the yardstick of mul"""
        r = None
        for bit in bin(k)[2:] if k else "":
            r = self.add(r, r)
            if bit == "1":
                r = self.add(r, P)
        return r

    def mul(self, k, P):
        """k P through Jacobian coordinates (x = X / Z^2, y = Y / Z^3; Z = 0 is the identity) with one inversion at the end; the
        textbook doubling for a = -3 and mixed addition, their special cases branched on"""
        p = self.p
        if P is None or k % self.n == 0:
            return None
        x2, y2 = P
        X, Y, Z = 0, 1, 0
        for bit in bin(k)[2:]:
            if Z:                                               # double
                zz = Z * Z % p
                m = 3 * (X - zz) * (X + zz) % p
                yy = Y * Y % p
                s = 4 * X * yy % p
                X3 = (m * m - 2 * s) % p
                Y, Z = (m * (s - X3) - 8 * yy * yy) % p, 2 * Y * Z % p
                X = X3
            if bit == "1":                                      # add the affine P
                if not Z:
                    X, Y, Z = x2, y2, 1
                    continue
                zz = Z * Z % p
                u2, s2 = x2 * zz % p, y2 * zz * Z % p
                h, r = (u2 - X) % p, (s2 - Y) % p
                if h == 0:
                    if r == 0:                                  # the same point: double it on the affine law
                        aff = self.add(P, P)
                        X, Y, Z = (0, 1, 0) if aff is None else (aff[0], aff[1], 1)
                    else:
                        X, Y, Z = 0, 1, 0
                    continue
                hh = h * h % p
                hhh, v = h * hh % p, X * hh % p
                X3 = (r * r - hhh - 2 * v) % p
                Y, Z = (r * (v - X3) - Y * hhh) % p, Z * h % p
                X = X3
        if not Z:
            return None
        zi = pow(Z, p - 2, p)
        return (X * zi * zi % p, Y * zi * zi * zi % p)

    def neg(self, P):
        return None if P is None else (P[0], -P[1] % self.p)

    # ---- SEC 1 2.3.3 / 2.3.4, compressed form only; the identity is the all-zero row ----------------------------------------
    def encode(self, P):
        if P is None:
            return bytes(self.Ne)
        return bytes([2 + (P[1] & 1)]) + P[0].to_bytes(self.Ns, "big")

    def decode(self, b):
        """the point, None for the identity (the zero row), or False for a row that is neither"""
        if len(b) != self.Ne:
            return False
        if b == bytes(self.Ne):
            return None
        x = int.from_bytes(b[1:], "big")
        if b[0] not in (2, 3) or x >= self.p:
            return False
        rhs = (x * x * x + self.a * x + self.b) % self.p
        y = pow(rhs, (self.p + 1) // 4, self.p)
        if y * y % self.p != rhs:
            return False
        return (x, y if y & 1 == b[0] & 1 else -y % self.p)

    # ---- RFC 9380 -------------------------------------------------------------------------------------------------------------
    def expand_message_xmd(self, msg, dst, n):
        """5.3.1; 1 <= len(dst) <= 255"""
        h = self.hash
        b_len, r_len = h().digest_size, h().block_size
        ell = -(-n // b_len)
        assert 1 <= len(dst) <= 255 and ell <= 255
        dst_prime = dst + bytes([len(dst)])
        b0 = h(bytes(r_len) + msg + n.to_bytes(2, "big") + b"\0" + dst_prime).digest()
        bi = h(b0 + b"\x01" + dst_prime).digest()
        out = bi
        for i in range(2, ell + 1):
            bi = h(bytes(x ^ y for x, y in zip(b0, bi)) + bytes([i]) + dst_prime).digest()
            out += bi
        return out[:n]

    def hash_to_field(self, msg, dst, count, modulus=None):
        u = self.expand_message_xmd(msg, dst, count * self.ell)
        return [int.from_bytes(u[i * self.ell:(i + 1) * self.ell], "big") % (modulus or self.p) for i in range(count)]

    def sswu_branch(self, u):
        """(gx1 is a square, sgn0(u)): the two selects of the map, for tests that must see both sides of each"""
        return self._sswu(u)[1], u % self.p & 1

    def _sswu(self, u):
        """F.2.1.2 sqrt_ratio_3mod4 inside F.2 simplified SWU, straight-line as the RFC states it"""
        p, A, B, Z = self.p, self.a, self.b, self.z
        u %= p
        tv1 = u * u % p
        tv3 = Z * tv1 % p
        tv2 = tv3 * tv3 % p
        xd = (tv2 + tv3) % p
        x1n = (xd + 1) * B % p
        xd = -A * xd % p
        if xd == 0:
            xd = Z * A % p
        tv2 = xd * xd % p
        gxd = tv2 * xd % p
        tv2 = A * tv2 % p
        gx1 = ((x1n * x1n + tv2) * x1n + B * gxd) % p
        tv4 = gxd * gxd % p
        tv2 = gx1 * gxd % p
        tv4 = tv4 * tv2 % p
        y1 = pow(tv4, self.c1, p) * tv2 % p
        x2n = tv3 * x1n % p
        y2 = y1 * self.c2 % p * tv1 % p * u % p
        e2 = y1 * y1 % p * gxd % p == gx1
        xn, y = (x1n, y1) if e2 else (x2n, y2)
        if u & 1 != y & 1:
            y = -y % p
        return (xn * pow(xd, p - 2, p) % p, y), e2

    def map_to_curve(self, u):
        pt = self._sswu(u)[0]
        assert self.on_curve(pt)
        return pt

    def hash_to_group_point(self, msg, dst, nonuniform=False):
        if nonuniform:
            return self.map_to_curve(self.hash_to_field(msg, dst, 1)[0])
        u0, u1 = self.hash_to_field(msg, dst, 2)
        return self.add(self.map_to_curve(u0), self.map_to_curve(u1))

    def hash_to_scalar_int(self, msg, dst):
        return self.hash_to_field(msg, dst, 1, self.n)[0]

    def decode_scalar(self, b):
        """the canonical scalar, or None for a value >= n"""
        k = int.from_bytes(b, "big")
        return k if len(b) == self.Ns and k < self.n else None

    def sc(self, k):
        return (k % self.n).to_bytes(self.Ns, "big")

    def context_string(self, mode):
        return b"OPRFV1-" + bytes([mode]) + b"-" + self.name.encode()


P256 = Curve(256, 2**256 - 2**224 + 2**192 + 2**96 - 1,
             0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b,
             0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551,
             0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
             0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5, -10,
             0x78bc71a02d89ec07214623f6d0f955072c7cc05604a5a6e23ffbf67115fa5301, "sha256", 48, "P256-SHA256")
P384 = Curve(384, 2**384 - 2**128 - 2**96 + 2**32 - 1,
             0xb3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875ac656398d8a2ed19d2a85c8edd3ec2aef,
             0xffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf581a0db248b0a77aecec196accc52973,
             0xaa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a385502f25dbf55296c3a545e3872760ab7,
             0x3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c00a60b1ce1d7e819d7a431d7c90ea0e5f, -12,
             0x19877cc1041b7555743c0ae2e3a3e61fb2aaa2e0e87ea557a563d8b598a0940d0a697a9e0b9e92cfaa314f583c9d066, "sha384", 72, "P384-SHA384")
CURVES = {256: P256, 384: P384}


# ---- the operations of the C ABI (curve = 256 or 384) -------------------------------------------------------------------------
def hash_to_group(curve, msg, dst, flags=0):
    c = CURVES[curve]
    return c.encode(c.hash_to_group_point(msg, dst, bool(flags & 1)))


def hash_to_scalar(curve, msg, dst):
    c = CURVES[curve]
    return c.sc(c.hash_to_scalar_int(msg, dst))


def scalar_mult(curve, scalar, elem=None, flags=0):
    """circl_hip_nistp_scalar_mult: (out, ok); elem None = the generator; flags & 1 = by the scalar's inverse; the identity is accepted"""
    c = CURVES[curve]
    k, p = c.decode_scalar(scalar), c.G if elem is None else c.decode(elem)
    if k is None or p is False or (flags & 1 and k == 0):
        return bytes(c.Ne), 0
    if flags & 1:
        k = pow(k, c.n - 2, c.n)
    return c.encode(c.mul(k, p)), 1


def derive_keypair(curve, mode, seed, info):
    """oprf/keys.go DeriveKey: (sk, pk, ok)"""
    c = CURVES[curve]
    if len(info) > 0xFFFF:
        return bytes(c.Ns), bytes(c.Ne), 0
    dst = b"DeriveKeyPair" + c.context_string(mode)
    for counter in range(256):
        sk = c.hash_to_scalar_int(seed + len(info).to_bytes(2, "big") + info + bytes([counter]), dst)
        if sk:
            return c.sc(sk), c.encode(c.mul(sk, c.G)), 1
    return bytes(c.Ns), bytes(c.Ne), 0


def _element(c, b):
    """RFC 9497 DeserializeElement: a valid encoding that is not the identity"""
    p = c.decode(b)
    return p if p else None


def _secret_scalar(c, b):
    k = c.decode_scalar(b)
    return k if k else None


def blind(curve, mode, inp, blind_bytes):
    """Client.DeterministicBlind: (blinded, ok)"""
    c = CURVES[curve]
    k = _secret_scalar(c, blind_bytes)
    if k is None or len(inp) > 0xFFFF:
        return bytes(c.Ne), 0
    out = c.mul(k, c.hash_to_group_point(inp, b"HashToGroup-" + c.context_string(mode)))
    return (c.encode(out), 1) if out is not None else (bytes(c.Ne), 0)


def evaluate(curve, sk, blinded):
    """base-mode Server.Evaluate: (evaluated, ok)"""
    c = CURVES[curve]
    k, p = _secret_scalar(c, sk), _element(c, blinded)
    if k is None or p is None:
        return bytes(c.Ne), 0
    return c.encode(c.mul(k, p)), 1


def _finalize_hash(c, inp, element):
    return c.hash(len(inp).to_bytes(2, "big") + inp + c.Ne.to_bytes(2, "big") + element + b"Finalize").digest()


def finalize(curve, inp, blind_bytes, evaluated):
    """base-mode Client.Finalize: (output, ok)"""
    c = CURVES[curve]
    k, p = _secret_scalar(c, blind_bytes), _element(c, evaluated)
    if k is None or p is None or len(inp) > 0xFFFF:
        return bytes(c.Nh), 0
    return _finalize_hash(c, inp, c.encode(c.mul(pow(k, c.n - 2, c.n), p))), 1


def full_evaluate(curve, mode, sk, inp):
    """Server.FullEvaluate (mode 0) / VerifiableServer.FullEvaluate (mode 1): (output, ok)"""
    assert mode in (0, 1)
    c = CURVES[curve]
    k = _secret_scalar(c, sk)
    if k is None or len(inp) > 0xFFFF:
        return bytes(c.Nh), 0
    element = c.mul(k, c.hash_to_group_point(inp, b"HashToGroup-" + c.context_string(mode)))
    return (_finalize_hash(c, inp, c.encode(element)), 1) if element is not None else (bytes(c.Nh), 0)


def poprf_scalar(curve, sk, info):
    """mode 2: the scalar whose INVERSE evaluates, skS + HashToScalar("Info" || I2OSP(len(info), 2) || info)"""
    c = CURVES[curve]
    m = c.hash_to_scalar_int(b"Info" + len(info).to_bytes(2, "big") + info, b"HashToScalar-" + c.context_string(2))
    return c.sc(int.from_bytes(sk, "big") + m)
