"""FrodoKEM-640-SHAKE in plain Python/numpy, restating the reference's kem/frodo/frodo640shake/{frodo,matrix_shake,noise,util}.go
word for word where the reference's behaviour is its own: A's words are the raw 16-bit SHAKE128 output, every product and sum
is taken mod 2^16, the 15-bit mask is applied only where the reference applies it, a private key's S words are arbitrary
uint16, and decapsulation uses the hpk stored in the key as it is.  Test infrastructure only: hashlib and numpy, no oracle/."""
import hashlib
import json
import os

import numpy as np

NAME = "FrodoKEM-640-SHAKE"
N, NBAR, LOGQ, B = 640, 8, 15, 2
QMASK = (1 << LOGQ) - 1
PK_BYTES, SK_BYTES, CT_BYTES, SS_BYTES, KEYSEED_BYTES, ENCSEED_BYTES = 9616, 19888, 9720, 16, 48, 16
BP_PACKED = LOGQ * N * NBAR // 8  # 9600
CDF = (4643, 13363, 20579, 25843, 29227, 31145, 32103, 32525, 32689, 32745, 32762, 32766, 32767)


def shake128(data, n):
    return hashlib.shake_128(bytes(data)).digest(n)


def _words(b):
    return np.frombuffer(bytes(b), "<u2").astype(np.uint16)


def sample(w):
    """noise.go sample: the 12-comparison sum, sign from bit 0, all in uint16."""
    w = np.asarray(w, np.uint16)
    sign = w & 1
    u = w >> 1
    g = np.zeros_like(w)
    for c in CDF[:-1]:
        g += (np.uint16(c) - u) >> 15
    return ((-sign.astype(np.int32)).astype(np.uint16) ^ g) + sign


def expand_a(seed_a):
    rows = [_words(shake128(bytes([i & 0xff, i >> 8]) + bytes(seed_a), 2 * N)) for i in range(N)]
    return np.stack(rows)  # (N, N) uint16, raw


def a_row(seed_a, i):
    return _words(shake128(bytes([i & 0xff, i >> 8]) + bytes(seed_a), 2 * N))


def _mm(x, y):
    """matrix product mod 2^16 (uint32 accumulation wraps consistently in its low 16 bits)"""
    return (x.astype(np.uint32) @ y.astype(np.uint32)).astype(np.uint16)


def pack(v):
    """util.go pack: 15-bit words, most significant bit first"""
    v = np.asarray(v, np.uint16).reshape(-1) & QMASK
    bits = ((v[:, None] >> np.arange(14, -1, -1, dtype=np.uint16)) & 1).astype(np.uint8)
    return np.packbits(bits.reshape(-1)).tobytes()


def unpack(b, n):
    bits = np.unpackbits(np.frombuffer(bytes(b), np.uint8))[: 15 * n].reshape(n, 15).astype(np.uint16)
    return (bits << np.arange(14, -1, -1, dtype=np.uint16)).sum(axis=1).astype(np.uint16)


def encode(mu):
    w = _words(mu)
    out = np.zeros(NBAR * NBAR, np.uint16)
    for i in range(8):
        for j in range(8):
            out[8 * i + j] = ((int(w[i]) >> (2 * j)) & 3) << (LOGQ - B)
    return out


def decode(m):
    m = np.asarray(m, np.uint16).reshape(-1)
    t = (((m & QMASK) + np.uint16(1 << (LOGQ - B - 1))) >> (LOGQ - B)) & 3
    out = bytearray(16)
    for i in range(16):
        for j in range(4):
            out[i] |= int(t[4 * i + j]) << (2 * j)
    return bytes(out)


def keygen(seed48):
    assert len(seed48) == KEYSEED_BYTES
    s, seed_se, z = seed48[:16], seed48[16:32], seed48[32:]
    seed_a = shake128(z, 16)
    r = sample(_words(shake128(b"\x5f" + seed_se, 4 * N * NBAR)))
    st = r[: N * NBAR].reshape(NBAR, N)       # transpose(S)
    e = r[N * NBAR:].reshape(N, NBAR)
    b = _mm(expand_a(seed_a), st.T) + e
    pk = seed_a + pack(b)
    sk = s + pk + st.astype("<u2").tobytes() + shake128(pk, 16)
    return pk, sk


def _encrypt(seed_a, b15, hpk, mu):
    """(packed B' || packed C, k) for the message mu under (seedA, B): shared by encaps and the re-encryption of decaps"""
    g2 = shake128(hpk + mu, 32)
    seed_se, k = g2[:16], g2[16:]
    r = sample(_words(shake128(b"\x96" + seed_se, 2 * (2 * N * NBAR + NBAR * NBAR))))
    sp = r[: N * NBAR].reshape(NBAR, N)
    ep = r[N * NBAR: 2 * N * NBAR].reshape(NBAR, N)
    epp = r[2 * N * NBAR:].reshape(NBAR, NBAR)
    bp = _mm(sp, expand_a(seed_a)) + ep
    v = (_mm(sp, b15.reshape(N, NBAR)) + epp) & QMASK
    c = (v.reshape(-1) + encode(mu)) & QMASK
    return pack(bp) + pack(c), k


def encaps(pk, mu):
    assert len(pk) == PK_BYTES and len(mu) == ENCSEED_BYTES
    ct, k = _encrypt(pk[:16], unpack(pk[16:], N * NBAR), shake128(pk, 16), bytes(mu))
    return ct, shake128(ct + k, 16)


def decaps(sk, ct):
    assert len(sk) == SK_BYTES and len(ct) == CT_BYTES
    s, pk = sk[:16], sk[16:16 + PK_BYTES]
    st = _words(sk[16 + PK_BYTES: 16 + PK_BYTES + 2 * N * NBAR]).reshape(NBAR, N)  # arbitrary uint16
    hpk = sk[-16:]                                                               # as stored
    bp = unpack(ct[:BP_PACKED], N * NBAR).reshape(NBAR, N)
    c = unpack(ct[BP_PACKED:], NBAR * NBAR)
    w = (c - (_mm(bp, st.T).reshape(-1) & QMASK)) & QMASK
    mu = decode(w)
    ct2, k = _encrypt(pk[:16], unpack(pk[16:], N * NBAR), hpk, mu)
    return shake128(ct + (k if ct2 == ct else s), 16)


# ---- the reference's pin: kem/frodo/kat_test.go ---------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frodo640shake.json")  # the recorded pin


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def kat_seeds(count):
    """(outer seed, key seed, encapsulation seed) of every KAT entry, as kat_test.go draws them"""
    from drbg import DRBG  # tests/drbg.py: AES through the system libcrypto, needed for the KAT replay only
    g = DRBG(bytes(range(48)))
    out = []
    for _ in range(count):
        seed = g.fill(48)
        g2 = DRBG(seed)
        out.append((seed, g2.fill(KEYSEED_BYTES), g2.fill(ENCSEED_BYTES)))
    return out


def kat_transcript(name, entries):
    """entries: (outer seed, pk, sk, ct, ss) per count"""
    f = hashlib.sha256()
    f.update(("# %s\n\n" % name).encode())
    for i, (seed, pk, sk, ct, ss) in enumerate(entries):
        f.update(("count = %d\n" % i).encode())
        for label, v in (("seed", seed), ("pk", pk), ("sk", sk), ("ct", ct)):
            f.update(("%s = %s\n" % (label, bytes(v).hex().upper())).encode())
        f.update(("ss = %s\n\n" % bytes(ss).hex().upper()).encode())
    return f.hexdigest()
