"""CPU checker for the ristretto255 group (RFC 9496), its hash-to-group / hash-to-scalar (RFC 9380 expand_message_xmd, SHA-512) and
the proof-free part of OPRF (RFC 9497, suite ristretto255-SHA512): big integers and hashlib, written from the RFCs.  The functions of the
second half take and return bytes and follow the C ABI (include/circl_hip.h) operation by operation, `ok` rules included: a failed
item is ok = 0 and zero rows.  It is the yardstick of the GPU tests; tests/test_oracle_oprf.py checks it against the fixture."""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
SQRT_AD_MINUS_ONE = 25063068953384623474111414158702152701244531502492656460079210482610430750235   # the ODD root of a d - 1
INVSQRT_A_MINUS_D = 54469307008909316920995813868745141605393597292927456921205312896311721017578
ONE_MINUS_D_SQ = (1 - D * D) % P
D_MINUS_ONE_SQ = (D - 1) ** 2 % P
assert SQRT_AD_MINUS_ONE ** 2 % P == (-D - 1) % P and SQRT_AD_MINUS_ONE & 1
assert INVSQRT_A_MINUS_D ** 2 * (-1 - D) % P == 1 and not INVSQRT_A_MINUS_D & 1

ZERO32, ZERO64 = bytes(32), bytes(64)


def is_neg(x):
    return x % P & 1


def ct_abs(x):
    return (-x if is_neg(x) else x) % P


def sqrt_ratio_m1(u, v):
    """RFC 9496 4.2: (was_square, the non-negative root of u / v or of SQRT_M1 u / v)"""
    u, v = u % P, v % P
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct, flipped, flipped_i = check == u, check == -u % P, check == -u * SQRT_M1 % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return correct or flipped, ct_abs(r)


# ---- points: extended coordinates (X, Y, Z, T) on -x^2 + y^2 = 1 + d x^2 y^2 -------------------------------------------------
IDENTITY = (0, 1, 1, 0)


def decode(b):
    """RFC 9496 4.3.1, strictly: None for s >= p, negative s, a non-square, negative t, y = 0"""
    if len(b) != 32:
        return None
    s = int.from_bytes(b, "little")
    if s >= P or s & 1:
        return None
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 * u1) - u2_sqr) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2_sqr)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x * v % P
    x = ct_abs(2 * s * den_x)
    y = u1 * den_y % P
    t = x * y % P
    if not was_square or is_neg(t) or y == 0:
        return None
    return (x, y, 1, t)


def encode(pt):
    """RFC 9496 4.3.2"""
    x0, y0, z0, t0 = pt
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2)
    den1, den2 = invsqrt * u1 % P, invsqrt * u2 % P
    z_inv = den1 * den2 * t0 % P
    if is_neg(t0 * z_inv):
        x, y, den_inv = y0 * SQRT_M1 % P, x0 * SQRT_M1 % P, den1 * INVSQRT_A_MINUS_D % P
    else:
        x, y, den_inv = x0, y0, den2
    if is_neg(x * z_inv):
        y = -y % P
    return ct_abs(den_inv * (z0 - y)).to_bytes(32, "little")


def add(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k, p):
    r = IDENTITY
    for bit in bin(k)[2:] if k else "":
        r = add(r, r)
        if bit == "1":
            r = add(r, p)
    return r


_BY = 4 * pow(5, P - 2, P) % P
_BX = sqrt_ratio_m1(_BY * _BY - 1, D * _BY * _BY + 1)[1]      # the even root: the Ed25519 base point
GENERATOR = (_BX, _BY, 1, _BX * _BY % P)


def elligator(t):
    """RFC 9496 4.3.4 MAP"""
    r = SQRT_M1 * t * t % P
    u = (r + 1) * ONE_MINUS_D_SQ % P
    v = (-1 - r * D) * (r + D) % P
    was_square, s = sqrt_ratio_m1(u, v)
    if not was_square:
        s, c = -ct_abs(s * t) % P, r
    else:
        c = P - 1
    n = (c * (r - 1) * D_MINUS_ONE_SQ - v) % P
    w0, w1, w2, w3 = 2 * s * v % P, n * SQRT_AD_MINUS_ONE % P, (1 - s * s) % P, (1 + s * s) % P
    return (w0 * w3 % P, w2 * w1 % P, w1 * w3 % P, w0 * w2 % P)


# ---- hashing ----------------------------------------------------------------------------------------------------------------
def expand_message_xmd(msg, dst, n=64):
    """RFC 9380 5.3.1 with SHA-512, for n <= 64 (one b_1); 1 <= len(dst) <= 255"""
    assert 1 <= len(dst) <= 255 and 0 < n <= 64
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha512(bytes(128) + msg + n.to_bytes(2, "big") + b"\0" + dst_prime).digest()
    return hashlib.sha512(b0 + b"\x01" + dst_prime).digest()[:n]


def hash_to_group_point(msg, dst):
    u = expand_message_xmd(msg, dst)
    t0, t1 = (int.from_bytes(h, "little") & (2**255 - 1) for h in (u[:32], u[32:]))
    return add(elligator(t0 % P), elligator(t1 % P))


def hash_to_group(msg, dst):
    return encode(hash_to_group_point(msg, dst))


def hash_to_scalar_int(msg, dst):
    return int.from_bytes(expand_message_xmd(msg, dst), "little") % L


def hash_to_scalar(msg, dst):
    return hash_to_scalar_int(msg, dst).to_bytes(32, "little")


def decode_scalar(b):
    """the canonical scalar, or None for a value >= L"""
    k = int.from_bytes(b, "little")
    return k if len(b) == 32 and k < L else None


# ---- the operations of the C ABI --------------------------------------------------------------------------------------------
def context_string(mode):
    return b"OPRFV1-" + bytes([mode]) + b"-ristretto255-SHA512"


def scalar_mult(scalar, elem=None, flags=0):
    """circl_hip_ristretto255_scalar_mult: (out, ok); elem None = the generator; flags & 1 = by the scalar's inverse"""
    k, p = decode_scalar(scalar), GENERATOR if elem is None else decode(elem)
    if k is None or p is None or (flags & 1 and k == 0):
        return ZERO32, 0
    if flags & 1:
        k = pow(k, L - 2, L)
    return encode(mul(k, p)), 1


def derive_keypair(mode, seed, info):
    """oprf/keys.go DeriveKey: (sk, pk, ok)"""
    if len(info) > 0xFFFF:
        return ZERO32, ZERO32, 0
    dst = b"DeriveKeyPair" + context_string(mode)
    for counter in range(256):
        sk = hash_to_scalar_int(seed + len(info).to_bytes(2, "big") + info + bytes([counter]), dst)
        if sk:
            return sk.to_bytes(32, "little"), encode(mul(sk, GENERATOR)), 1
    return ZERO32, ZERO32, 0


def _element(b):
    """RFC 9497 DeserializeElement: a valid encoding that is not the identity"""
    return None if b == ZERO32 else decode(b)


def _secret_scalar(b):
    k = decode_scalar(b)
    return k if k else None


def blind(mode, inp, blind_bytes):
    """Client.DeterministicBlind: (blinded, ok)"""
    k = _secret_scalar(blind_bytes)
    if k is None or len(inp) > 0xFFFF:
        return ZERO32, 0
    out = encode(mul(k, hash_to_group_point(inp, b"HashToGroup-" + context_string(mode))))
    return (out, 1) if out != ZERO32 else (ZERO32, 0)


def evaluate(sk, blinded):
    """base-mode Server.Evaluate: (evaluated, ok)"""
    k, p = _secret_scalar(sk), _element(blinded)
    if k is None or p is None:
        return ZERO32, 0
    return encode(mul(k, p)), 1


def _finalize_hash(inp, element):
    return hashlib.sha512(len(inp).to_bytes(2, "big") + inp + (32).to_bytes(2, "big") + element + b"Finalize").digest()


def finalize(inp, blind_bytes, evaluated):
    """base-mode Client.Finalize: (output, ok)"""
    k, p = _secret_scalar(blind_bytes), _element(evaluated)
    if k is None or p is None or len(inp) > 0xFFFF:
        return ZERO64, 0
    return _finalize_hash(inp, encode(mul(pow(k, L - 2, L), p))), 1


def full_evaluate(mode, sk, inp):
    """Server.FullEvaluate (mode 0) / VerifiableServer.FullEvaluate (mode 1): (output, ok)"""
    assert mode in (0, 1)
    k = _secret_scalar(sk)
    if k is None or len(inp) > 0xFFFF:
        return ZERO64, 0
    element = encode(mul(k, hash_to_group_point(inp, b"HashToGroup-" + context_string(mode))))
    return (_finalize_hash(inp, element), 1) if element != ZERO32 else (ZERO64, 0)


def poprf_scalar(sk, info):
    """mode 2: the scalar whose INVERSE evaluates, skS + HashToScalar("Info" || I2OSP(len(info), 2) || info), as 32 bytes"""
    m = hash_to_scalar_int(b"Info" + len(info).to_bytes(2, "big") + info, b"HashToScalar-" + context_string(2))
    return ((int.from_bytes(sk, "little") + m) % L).to_bytes(32, "little")
