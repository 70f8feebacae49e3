"""RFC 7748 X448 and RFC 8032 section 5.2 Ed448 (pure, with context) in plain Python: the checker for the Curve448 tests (the
product side runs on the GPU; the reference uses dh/x448, sign/ed448 and ecc/goldilocks).  Written from the RFCs with hashlib's
shake_256 and Python integers, on the untwisted Edwards curve x^2 + y^2 = 1 + d x^2 y^2, d = -39081.  Test infrastructure only.

Verification has three named rules (RULES):
  "circl"         what sign/ed448 computes: goldilocks.Curve.CombinedMult divides both scalars by 4 mod l, works on a 4-isogenous
                  curve and comes back, which multiplies by 4: Q = 4 ([S/4 mod l]B + [k/4 mod l](-A)), then enc(Q) == R.  The
                  4-torsion component of A drops out; one of R does not.
  "cofactorless"  enc([S]B - [k]A) == R
  "cofactored"    RFC 8032 5.2.7: R decodes and [4][S]B == [4]R + [4][k]A
"""
import hashlib

P = 2**448 - 2**224 - 1
L = 2**446 - 13818066809895115352007386748515426880336692474882178609894547503885
D = -39081 % P
A24 = 39081


def _h(*parts):
    return hashlib.shake_256(b"".join(parts)).digest(114)


def dom4(ctx: bytes, ph: int = 0) -> bytes:
    return b"SigEd448" + bytes([ph, len(ctx)]) + ctx


# ---- X448 -----------------------------------------------------------------------------------------------------------------
def x448_raw(k: int, u: int) -> int:
    """the RFC 7748 ladder for an already-clamped scalar k and a u-coordinate below p"""
    x1, x2, z2, x3, z3, swap = u, 1, 0, u, 1, 0
    for t in range(447, -1, -1):
        kt = (k >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2 * pow(z2, P - 2, P) % P


def clamp448(scalar: bytes) -> int:
    k = bytearray(scalar)
    k[0] &= 252
    k[55] |= 128
    return int.from_bytes(k, "little")


def x448(scalar: bytes, point: bytes = None):
    """(out, ok) as dh/x448 Shared: the point is reduced mod p, ok is False for u in {0, 1, p - 1}; point None: KeyGen (u = 5)"""
    u = 5 if point is None else int.from_bytes(point, "little") % P
    return x448_raw(clamp448(scalar), u).to_bytes(56, "little"), u not in (0, 1, P - 1)


# ---- the Edwards curve ----------------------------------------------------------------------------------------------------
def add(p, q):  # extended coordinates (X, Y, Z, T), a = 1; complete (d is not a square)
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b, c, d = x1 * x2 % P, y1 * y2 % P, D * t1 * t2 % P, z1 * z2 % P
    e = ((x1 + y1) * (x2 + y2) - a - b) % P
    f, g, h = d - c, d + c, b - a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k, p):
    q = (0, 1, 1, 0)
    while k:
        if k & 1:
            q = add(q, p)
        p = add(p, p)
        k >>= 1
    return q


def neg(p):
    return ((P - p[0]) % P, p[1], p[2], (P - p[3]) % P)


def affine(p):
    zi = pow(p[2], P - 2, P)
    return p[0] * zi % P, p[1] * zi % P


def from_affine(x, y):
    return (x % P, y % P, 1, x * y % P)


def sqrt_ratio(u, v):
    """(is_square, x) with v x^2 == u when u / v is a square (the reference's fp.InvSqrt: exponent (p - 3) / 4)"""
    x = u * u * u * v % P * pow(pow(u, 5, P) * pow(v, 3, P) % P, (P - 3) // 4, P) % P
    return (v * x * x - u) % P == 0, x


def _recover_x(y, sign):
    if y >= P:
        return None
    ok, x = sqrt_ratio((y * y - 1) % P, (D * y * y - 1) % P)
    if not ok:
        return None
    if x == 0 and sign:
        return None
    if x & 1 != sign:
        x = (P - x) % P
    return x


BY = 298819210078481492676017930443930673437544040154080242095928241372331506189835876003536878655418784733982303233503462500531545062832660
BX = 224580040295924300187604334099896036246789641632564134246125461686950415467406032909029192869357953282578032075146446173674602635247710
B = from_affine(BX, BY)
T4 = (1, 0, 1, 0)        # order 4
T2 = (0, P - 1, 1, 0)    # order 2
IDENTITY = (0, 1, 1, 0)


def encode(p) -> bytes:
    x, y = affine(p)
    return (y | ((x & 1) << 455)).to_bytes(57, "little")


def decode(s: bytes):
    """the point, or None where ecc/goldilocks point.go FromBytes rejects the encoding"""
    if len(s) != 57 or s[56] & 0x7F:
        return None
    y = int.from_bytes(s[:56], "little")
    x = _recover_x(y, s[56] >> 7)
    return None if x is None else from_affine(x, y)


def _expand(seed):
    h = bytearray(_h(seed))
    h[0] &= 0xFC
    h[55] |= 0x80
    h[56] = 0
    return int.from_bytes(h[:57], "little"), bytes(h[57:])


def public(seed: bytes) -> bytes:
    return encode(mul(_expand(seed)[0], B))


def sign_parts(sk: bytes, msg: bytes, ctx: bytes = b""):
    """(r, k, s, signature); sk = seed || A (114 bytes), the A half hashed as given, as sign/ed448 does"""
    s, prefix = _expand(sk[:57])
    d4 = dom4(ctx)
    r = int.from_bytes(_h(d4, prefix, msg), "little") % L
    R = encode(mul(r, B))
    k = int.from_bytes(_h(d4, R, sk[57:], msg), "little") % L
    return r, k, s, R + ((r + k * s) % L).to_bytes(57, "little")


def sign(sk: bytes, msg: bytes, ctx: bytes = b"") -> bytes:
    return sign_parts(sk, msg, ctx)[3]


def challenge(R: bytes, pk: bytes, msg: bytes, ctx: bytes = b"") -> int:
    return int.from_bytes(_h(dom4(ctx), R, pk, msg), "little") % L


def combined_circl(s: int, k: int, q):
    """what goldilocks.Curve.CombinedMult(s, k, q) returns: 4 ([s/4]B + [k/4]q)"""
    inv4 = pow(4, L - 2, L)
    return mul(4, add(mul(s * inv4 % L, B), mul(k * inv4 % L, q)))


def _rule_circl(s, k, A, R):
    return encode(combined_circl(s, k, neg(A))) == R


def _rule_cofactorless(s, k, A, R):
    return encode(add(mul(s, B), mul(k, neg(A)))) == R


def _rule_cofactored(s, k, A, R):
    Rp = decode(R)
    if Rp is None:
        return False
    return affine(mul(4 * s, B)) == affine(add(mul(4, Rp), mul(4 * k, A)))


RULES = {"circl": _rule_circl, "cofactorless": _rule_cofactorless, "cofactored": _rule_cofactored}


def verify(pk: bytes, msg: bytes, sig: bytes, ctx: bytes = b"", rule: str = "circl") -> bool:
    if len(pk) != 57 or len(sig) != 114 or len(ctx) > 255:
        return False
    s = int.from_bytes(sig[57:], "little")  # isLessThanOrder: byte 56 is part of the number, so it must be 0
    if s >= L:
        return False
    A = decode(pk)
    if A is None:
        return False
    return RULES[rule](s, challenge(sig[:57], pk, msg, ctx), A, sig[:57])


def y_without_x() -> int:
    """the smallest y >= 2 for which no x exists on the curve (a reject of decode)"""
    y = 2
    while _recover_x(y, 0) is not None:
        y += 1
    return y


def base_mult(k: int) -> bytes:
    return encode(mul(k, B))
