"""RFC 8032 section 5.1 Ed25519 (pure) in plain Python: the checker for the Ed25519 tests (the product side runs on the GPU;
the reference uses sign/ed25519).  Written from the RFC with hashlib's sha512 and Python integers.  Test infrastructure only."""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def _h(*parts):
    return hashlib.sha512(b"".join(parts)).digest()


def _add(p, q):  # extended coordinates (X, Y, Z, T), a = -1 (RFC 8032 5.1.4)
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * t1 * t2 * D % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def _mul(k, p):
    q = (0, 1, 1, 0)
    while k:
        if k & 1:
            q = _add(q, p)
        p = _add(p, p)
        k >>= 1
    return q


def _recover_x(y, sign):
    if y >= P:
        return None
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    if x2 == 0:
        return None if sign else 0
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRT_M1 % P
    if (x * x - x2) % P:
        return None
    if x & 1 != sign:
        x = P - x
    return x


_BY = 4 * pow(5, P - 2, P) % P
_BX = _recover_x(_BY, 0)
B = (_BX, _BY, 1, _BX * _BY % P)


def encode(p):
    x, y, z, _ = p
    zi = pow(z, P - 2, P)
    x, y = x * zi % P, y * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(s: bytes):
    """the point, or None where RFC 8032 5.1.3 (and point.go FromBytes) rejects the encoding"""
    v = int.from_bytes(s, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    x = _recover_x(y, sign)
    return None if x is None else (x, y, 1, x * y % P)


def _expand(seed):
    h = _h(seed)
    a = int.from_bytes(h[:32], "little")
    a &= (1 << 254) - 8
    a |= 1 << 254
    return a, h[32:]


def public(seed: bytes) -> bytes:
    return encode(_mul(_expand(seed)[0], B))


def sign(sk: bytes, msg: bytes) -> bytes:
    """sk = seed || A (64 bytes); the A half is hashed as given, as sign/ed25519 does"""
    a, prefix = _expand(sk[:32])
    r = int.from_bytes(_h(prefix, msg), "little") % L
    R = encode(_mul(r, B))
    k = int.from_bytes(_h(R, sk[32:], msg), "little") % L
    return R + ((r + k * a) % L).to_bytes(32, "little")


def verify(pk: bytes, msg: bytes, sig: bytes) -> bool:
    """cofactorless: enc([S]B - [k]A) == R, as sign/ed25519's verify"""
    if len(pk) != 32 or len(sig) != 64:
        return False
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return False
    A = decode(pk)
    if A is None:
        return False
    k = int.from_bytes(_h(sig[:32], pk, msg), "little") % L
    negA = ((P - A[0]) % P, A[1], A[2], (P - A[3]) % P)
    return encode(_add(_mul(s, B), _mul(k, negA))) == sig[:32]


def double_scalar(s: int, k: int, pk: bytes) -> bytes:
    """enc([s]B + [k](-A)) for a decodable pk (the hostsim check of the device's joint multiplication)"""
    A = decode(pk)
    negA = ((P - A[0]) % P, A[1], A[2], (P - A[3]) % P)
    return encode(_add(_mul(s, B), _mul(k, negA)))


def base_mult(k: int) -> bytes:
    return encode(_mul(k, B))
