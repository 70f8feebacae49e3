"""Inputs at the ends of their ranges, shared by tests/test_oracle_rare_paths.py (which checks them and the oracle against plain
integer arithmetic) and the GPU tests tests/test_gpu_rare_paths.py / tests/test_gpu_mldsa_extremes.py (which pin the HIP kernels to the
oracle on them): encapsulation keys whose t^ is saturated, and ML-DSA private keys whose s1, s2 (and t0) are.  Plain numpy and hashlib;
of the oracle only the samplers (kyber_uniform, kyber_noise, dilithium_uniform)."""
import hashlib

import numpy as np

from oracle import orc

KQ = 3329
DQ = 8380417
KEM = {512: (2, 3, 10, 4), 768: (3, 2, 10, 4), 1024: (4, 2, 11, 5)}          # K, eta1, du, dv
DSA = {44: (4, 4, 2, 64), 65: (6, 5, 4, 64), 87: (8, 7, 2, 64), 2: (4, 4, 2, 32), 3: (6, 5, 4, 32), 5: (8, 7, 2, 32)}  # K, L, eta, tr bytes


def pack_bits(values, d):
    """d-bit little-endian packing of a flat array of non-negative integers (the layout of every Kyber / Dilithium byte encoding)"""
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    bits = ((v[:, None] >> np.arange(d)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def unpack_bits(buf, d):
    bits = np.unpackbits(np.frombuffer(bytes(buf), np.uint8), bitorder="little").reshape(-1, d).astype(np.int64)
    return (bits << np.arange(d)).sum(axis=1)


def brv(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


# ---- sampler streams, as the generator of tests/golden/rare_paths.json.gz counts them (tests/test_oracle_rare_paths.py counts them again,
# byte by byte, on its own) ---------------------------------------------------------------------------------------------------------------
def dsa_rhoprime(param, xi):
    """rho' of ML-DSA / Dilithium key generation: bytes 32..95 of SHAKE256(xi || K || L), round 3 hashes xi alone (dilithium.go:189-195)"""
    K, L = DSA[param][:2]
    return hashlib.shake_256(xi + (bytes([K, L]) if param > 10 else b"")).digest(128)[32:96]


def accepted_nibbles(param, rhoprime, nonce, blocks):
    """how many nibbles of the first `blocks` SHAKE256 blocks of the secret polynomial `nonce` are accepted (<= 8 at eta 4, <= 14 at eta 2)"""
    buf = np.frombuffer(hashlib.shake_256(rhoprime + bytes([nonce & 255, nonce >> 8])).digest(136 * blocks), np.uint8)
    lim = 8 if DSA[param][2] == 4 else 14
    return int((buf & 15 <= lim).sum() + (buf >> 4 <= lim).sum())


def kem_rho(scheme, K, d):
    """rho of a key made from d: SHA3-512(d || K) for ML-KEM ("mlkem"), SHA3-512(d) for round-3 Kyber ("kyber")"""
    return hashlib.sha3_512(d + (bytes([K]) if scheme == "mlkem" else b"")).digest()[:32]


def accepted_in_3_blocks(rho, x, y):
    """how many of the 336 candidates in three SHAKE128 blocks of XOF(rho || x || y) are below q"""
    b = np.frombuffer(hashlib.shake_128(rho + bytes([x, y])).digest(504), np.uint8).astype(np.uint16).reshape(-1, 3)
    t1 = (b[:, 0] | (b[:, 1] << 8)) & 0xFFF
    t2 = (b[:, 1] >> 4) | (b[:, 2] << 4)
    return int((t1 < KQ).sum() + (t2 < KQ).sum())


def ordinary_kem_seeds(scheme, param, n):
    """n keygen seeds d || z none of whose K^2 matrix streams needs a fourth block: SHA3-512("ordinary <scheme> <param> <k>") for
    increasing k, passing over the (about K^2 * 0.84 %) that do"""
    K = KEM[param][0]
    out, k = [], 0
    while len(out) < n:
        seed = hashlib.sha3_512(b"ordinary %s %d %d" % (scheme.encode(), param, k)).digest()
        k += 1
        rho = kem_rho(scheme, K, seed[:32])
        if all(accepted_in_3_blocks(rho, x, y) >= 256 for x in range(K) for y in range(K)):
            out.append(seed)
    return out


def kem_only_the_ends(scheme, param, fix):
    """the batch of 66 in which exactly items 0 and 65 have a fourth-block stream -> (seeds (66, 64), rho expected per item or None);
    fix = the fixture's kem_fourth_block[scheme][K]"""
    n = 66
    seeds = [bytes.fromhex(fix["multi"]["seed"])] + ordinary_kem_seeds(scheme, param, n - 2) + [bytes.fromhex(fix["exactly_255"]["seed"])]
    return np.frombuffer(b"".join(seeds), np.uint8).reshape(n, 64).copy(), [fix["multi"]["rho"]] + [None] * (n - 2) + [fix["exactly_255"]["rho"]]


def ordinary_dsa_seeds(param, n, tag):
    """n ML-DSA keygen seeds none of whose secret polynomials needs a third SHAKE256 block (eta = 4: about 1 key in 10^4 does; at
    eta = 2 two blocks always do) -- the neighbours of the rare seeds in a mixed batch"""
    K, L, eta = DSA[param][:3]
    out, k = [], 0
    while len(out) < n:
        xi = hashlib.sha3_256(b"ordinary dsa %d %d %d" % (param, tag, k)).digest()
        k += 1
        rp = dsa_rhoprime(param, xi)
        if eta == 2 or all(accepted_nibbles(param, rp, nonce, 2) >= 256 for nonce in range(K + L)):
            out.append(xi)
    return out


def dsa_mixed_batch(param, n, placed, tag):
    """n ordinary seeds with the rare seeds `placed` = [(position, xi)] put among them -> (n, 32)"""
    seeds = ordinary_dsa_seeds(param, n, tag)
    for place, xi in placed:
        seeds[place] = xi
    return np.frombuffer(b"".join(seeds), np.uint8).reshape(n, 32).copy()


def dsa_rare_seeds(fix, param):
    """the fixture's keygen seeds of a parameter set: third-block seeds (65, 3), block-1 boundary seeds (44, 87)"""
    if param in (65, 3):
        return [bytes.fromhex(h["xi"]) for h in fix["eta4_third_block"][str(param)]]
    f = fix["eta2_second_block"][str(param)]
    return [bytes.fromhex(h["xi"]) for kind in ("inside_block1", "exactly_256", "exactly_255") for h in f[kind]]


def dsa_mixed_batches(fix, param):
    """the rare seeds among ordinary ones: four at a time at positions 0, 63, 64, 69 of a batch of 70 (both ends of a wavefront's items
    and of the batch), and all of them in one batch of 600 -- more than 2^9 keys leave the one-launch kernel (a workgroup per key) for
    the kernel that samples the streams of several keys on the lanes of one wavefront -- at both ends, around item 64 and side by side
    -> [(seeds, [(position, xi)])]"""
    special = dsa_rare_seeds(fix, param)
    out = []
    for b in range(0, len(special), 4):
        put = list(zip((0, 63, 64, 69), special[b:b + 4]))
        out.append((dsa_mixed_batch(param, 70, put, b), put))
    put = list(zip([0, 63, 64, 599] + list(range(300, 300 + len(special))), special[:4] + special))
    out.append((dsa_mixed_batch(param, 600, put, 600), put))
    return out


# ---- saturated encapsulation keys -------------------------------------------------------------------------------------------------------
EK_FAMILIES = ("all_3328", "all_0", "odd_coefficients_3328", "alternate_polynomials_3328", "even_registers_3328", "all_1664")
EK_REFUSED = ("all_3329", "all_4095")                     # ML-KEM: kem.ErrPubKey; round-3 Kyber reduces them (and all_3330)
EK_NONCANONICAL = ("all_4095", "all_3329", "all_3330")


def ek_that(family, K):
    """the K x 256 coefficients of t^ of a family"""
    t = np.zeros((K, 256), np.int64)
    if family.startswith("all_"):
        t[:] = int(family[4:])
    elif family == "odd_coefficients_3328":               # 0, 3328, 0, 3328, ...
        t[:, 1::2] = 3328
    elif family == "alternate_polynomials_3328":          # polynomial 0 full, 1 empty, ...
        t[0::2] = 3328
    elif family == "even_registers_3328":                 # coefficients 4l and 4l + 2: a lane's registers 0 and 2
        t[:, 0::2] = 3328
    else:
        raise KeyError(family)
    return t


def saturated_ek(param, family, rho):
    K = KEM[param][0]
    return pack_bits(ek_that(family, K), 12) + bytes(rho)


def _kyber_roots():
    return [pow(17, 2 * brv(i, 7) + 1, KQ) for i in range(128)]


_KYBER_M = {}


def kyber_ntt_exact(f, inverse=False):
    """FIPS 203 NTT by its definition: f^[2i] + f^[2i+1] X = f mod (X^2 - 17^(2 brv7(i) + 1)); exact integers, no Montgomery factors"""
    f = np.asarray(f, dtype=np.int64) % KQ
    if inverse not in _KYBER_M:
        w = _kyber_roots()
        if not inverse:
            M = [[pow(w[i], j, KQ) for j in range(128)] for i in range(128)]
        else:
            n_inv = pow(128, -1, KQ)
            M = [[n_inv * pow(w[i], -j, KQ) % KQ for i in range(128)] for j in range(128)]
        _KYBER_M[inverse] = np.array(M, dtype=np.int64)
    M = _KYBER_M[inverse]
    out = np.empty(256, np.int64)
    out[0::2] = M @ f[0::2] % KQ
    out[1::2] = M @ f[1::2] % KQ
    return out


_IDX = np.arange(256)[:, None] - np.arange(256)[None, :]


def negacyclic(a, b, q):
    """schoolbook a * b mod (X^256 + 1, q): r[k] = sum_i a[i] * (+-b[k - i]), the sign flipping where k - i wraps; |a b| * 256 < 2^63"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    return np.where(_IDX >= 0, b[_IDX % 256], -b[_IDX % 256]) @ a % q


def _signed(p):
    return np.asarray(p, dtype=np.int64)


def kpke_encrypt_direct(param, ek, m, coins):
    """K-PKE.Encrypt (FIPS 203 algorithm 14) with schoolbook products in Z_q[X]/(X^256 + 1): t and A are brought out of the NTT domain by
    the definition of the transform, everything else is integers mod q.  Coefficients of t^ are taken mod q (round-3 Kyber's rule; ML-KEM
    refuses the others before it gets here).  Shares only the oracle's samplers."""
    K, eta1, du, dv = KEM[param]
    ek = bytes(ek)
    that = unpack_bits(ek[:384 * K], 12).reshape(K, 256) % KQ
    rho = ek[384 * K:]
    t = [kyber_ntt_exact(that[i], inverse=True) for i in range(K)]
    r = [_signed(orc.kyber_noise(coins, i, eta1)) for i in range(K)]
    e1 = [_signed(orc.kyber_noise(coins, K + i, 2)) for i in range(K)]
    e2 = _signed(orc.kyber_noise(coins, 2 * K, 2))
    out = b""
    for i in range(K):
        u = e1[i].copy()
        for j in range(K):
            a_t = kyber_ntt_exact(_signed(orc.kyber_uniform(rho, i, j)), inverse=True)   # A^T[i][j] = A[j][i]: XOF(rho || i || j)
            u = u + negacyclic(a_t, r[j], KQ)
        out += pack_bits((((u % KQ) << du) + KQ // 2) // KQ % (1 << du), du)
    v = e2 + 1665 * np.unpackbits(np.frombuffer(bytes(m), np.uint8), bitorder="little").astype(np.int64)
    for j in range(K):
        v = v + negacyclic(t[j], r[j], KQ)
    return out + pack_bits((((v % KQ) << dv) + KQ // 2) // KQ % (1 << dv), dv)


def mlkem_encaps_direct(param, ek, m):
    g = hashlib.sha3_512(bytes(m) + hashlib.sha3_256(bytes(ek)).digest()).digest()
    return kpke_encrypt_direct(param, ek, m, g[32:]), g[:32]


def kyber_r3_encaps_direct(param, ek, seed):
    m = hashlib.sha3_256(bytes(seed)).digest()
    g = hashlib.sha3_512(m + hashlib.sha3_256(bytes(ek)).digest()).digest()
    ct = kpke_encrypt_direct(param, ek, m, g[32:])
    return ct, hashlib.shake_256(g[:32] + hashlib.sha3_256(ct).digest()).digest(32)


# ---- saturated ML-DSA private keys ------------------------------------------------------------------------------------------------------
def _mulmod(M, v):
    """M @ v mod q for entries below 2^23 without leaving int64: v in 12-bit halves"""
    lo, hi = v & 0xFFF, v >> 12
    return ((M @ lo) % DQ + ((M @ hi) % DQ << 12)) % DQ


_DIL_M = {}


def dilithium_ntt_exact(f, inverse=False):
    """a^[k] = a(1753^(2 brv8(k) + 1)) (FIPS 204 section 7.5 order); exact, without the reference's Montgomery factor"""
    f = np.asarray(f, dtype=np.int64) % DQ
    if inverse not in _DIL_M:
        e = [2 * brv(k, 8) + 1 for k in range(256)]
        pw = [pow(1753, x, DQ) for x in range(512)]
        if not inverse:
            M = [[pw[e[k] * j % 512] for j in range(256)] for k in range(256)]
        else:
            n_inv = pow(256, -1, DQ)
            M = [[n_inv * pw[-e[k] * j % 512] % DQ for k in range(256)] for j in range(256)]
        _DIL_M[inverse] = np.array(M, dtype=np.int64)
    return _mulmod(_DIL_M[inverse], f)


S_FILLS = ("plus_eta", "minus_eta", "alternating")


def saturated_s(param, fill):
    K, L, eta, _ = DSA[param]
    s = np.full((L + K, 256), eta, np.int64)
    if fill == "minus_eta":
        s = -s
    elif fill == "alternating":
        s[:, 1::2] = -eta
    return s[:L], s[L:]


def mldsa_key_from_s(param, s1, s2, rho=None, key=None, t0_override=None):
    """(pk, sk) of the key with the given secret vectors, built from FIPS 204 algorithm 6 with integers: A from ExpandA (the oracle's
    sampler, taken out of the NTT domain by the transform's definition), t = A s1 + s2 by negacyclic convolution, Power2Round, the
    packings, tr = H(pk).  t0_override: every t0 coefficient set to that value in sk only (no public key matches it then)."""
    K, L, eta, TR = DSA[param]
    rho = hashlib.sha3_256(b"saturated key rho %d" % param).digest() if rho is None else rho
    key = hashlib.sha3_256(b"saturated key K %d" % param).digest() if key is None else key
    t = np.zeros((K, 256), np.int64)
    for i in range(K):
        acc = np.asarray(s2[i], np.int64).copy()
        for j in range(L):
            a = dilithium_ntt_exact(orc.dilithium_uniform(rho, (i << 8) + j), inverse=True)
            acc = (acc + negacyclic(a, s1[j], DQ)) % DQ                   # |s| <= 15, a < 2^23, 256 terms: below 2^35
        t[i] = acc % DQ
    t0 = t & 8191
    t0 = np.where(t0 > 4096, t0 - 8192, t0)                               # in (-2^12, 2^12]
    t1 = (t - t0) >> 13
    pk = rho + pack_bits(t1, 10)
    tr = hashlib.shake_256(pk).digest(TR)
    if t0_override is not None:
        t0 = np.full_like(t0, t0_override)
    d = 3 if eta == 2 else 4
    sk = rho + key + tr + pack_bits(eta - np.asarray(s1), d) + pack_bits(eta - np.asarray(s2), d) + pack_bits(4096 - t0, 13)
    assert len(pk) == orc.DSA_SIZES[param][0] and len(sk) == orc.DSA_SIZES[param][1]
    return pk, sk


def sk_with_eta_codes(param, sk, code, every):
    """sk with the packed code of s1 / s2 coefficients replaced by `code` (0 .. 2^bits - 1; codes above 2 eta are non-canonical):
    every `every`-th coefficient, 1 = all of them"""
    K, L, eta, TR = DSA[param]
    d = 3 if eta == 2 else 4
    off, size = 64 + TR, 32 * d * (K + L)
    codes = unpack_bits(sk[off:off + size], d)
    codes[::every] = code
    return sk[:off] + pack_bits(codes, d) + sk[off + size:]


def sk_with_t0_bytes(param, sk, byte):
    """every t0 coefficient 2^12 (byte 0x00: the 13-bit field 2^12 - t0 = 0) or -2^12 + 1 (0xFF: the field 8191)"""
    K = DSA[param][0]
    return sk[:len(sk) - 416 * K] + bytes([byte]) * (416 * K)


def signable(param, sk, want, tag=b"extreme"):
    """the first `want` messages b"<tag> <k>" the oracle signs with sk in fewer than 200 attempts -> (msgs, attempts)"""
    msgs, atts, k = [], [], 0
    while len(msgs) < want:
        m = tag + b" %d" % k
        k += 1
        tr = orc.mldsa_sign_trace(param, sk, m)
        if tr is not None and tr[1] < 200:
            msgs.append(m)
            atts.append(tr[1])
    return msgs, atts
