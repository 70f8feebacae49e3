"""The test suite's checker for the Ascon AEADs: plain Python following cipher/ascon/ascon.go step by step (Ascon v1.2: Ascon128,
Ascon128a, Ascon80pq).  tests/test_oracle_ascon.py checks it against every vector of tests/golden/ascon.json.gz."""
ASCON128, ASCON128A, ASCON80PQ = 1, 2, -1
MODES = {"Ascon128": ASCON128, "Ascon128a": ASCON128A, "Ascon80pq": ASCON80PQ}
PERM_A, TAG_SIZE, NONCE_SIZE = 12, 16, 16
M64 = (1 << 64) - 1


def key_size(mode):
    return {ASCON128: 16, ASCON128A: 16, ASCON80PQ: 20}[mode]


def block_size(mode):
    return abs(mode) << 3


def perm_b(mode):
    return (abs(mode) + 2) << 1


def _ror(x, n):
    return (x >> n | x << (64 - n)) & M64


def perm(n, s):
    x0, x1, x2, x3, x4 = s
    for i in range(PERM_A - n, PERM_A):
        x2 ^= (0xF - i) << 4 | i
        x0 ^= x4; x4 ^= x3; x2 ^= x1
        t0 = x0 & ~x4
        x0 ^= x2 & ~x1
        x2 ^= x4 & ~x3
        x4 ^= x1 & ~x0
        x1 ^= x3 & ~x2
        x3 ^= t0
        x1 ^= x0; x3 ^= x2; x0 ^= x4
        x2 = ~x2 & M64
        x0 ^= _ror(x0, 19) ^ _ror(x0, 28)
        x1 ^= _ror(x1, 61) ^ _ror(x1, 39)
        x2 ^= _ror(x2, 1) ^ _ror(x2, 6)
        x3 ^= _ror(x3, 10) ^ _ror(x3, 17)
        x4 ^= _ror(x4, 7) ^ _ror(x4, 41)
    s[:] = [x0, x1, x2, x3, x4]


def _key_words(mode, key):
    assert len(key) == key_size(mode)
    be = lambda b: int.from_bytes(b, "big")
    return [be(key[0:4]), be(key[4:12]), be(key[12:20])] if mode == ASCON80PQ else [0, be(key[0:8]), be(key[8:16])]


def _initialize(mode, k, nonce):
    assert len(nonce) == NONCE_SIZE
    s = [key_size(mode) * 8 << 56 | block_size(mode) * 8 << 48 | PERM_A << 40 | perm_b(mode) << 32 | k[0], k[1], k[2],
         int.from_bytes(nonce[:8], "big"), int.from_bytes(nonce[8:], "big")]
    perm(PERM_A, s)
    s[2] ^= k[0]; s[3] ^= k[1]; s[4] ^= k[2]
    return s


def _assoc_data(mode, s, add):
    bcs, pb = block_size(mode), perm_b(mode)
    if add:
        while len(add) >= bcs:
            for i in range(0, bcs, 8):
                s[i // 8] ^= int.from_bytes(add[i:i + 8], "big")
            perm(pb, s)
            add = add[bcs:]
        for i, b in enumerate(add):
            s[i // 8] ^= b << (56 - 8 * (i % 8))
        s[len(add) // 8] ^= 0x80 << (56 - 8 * (len(add) % 8))
        perm(pb, s)
    s[4] ^= 1


def _proc_text(mode, s, text, enc):
    bcs, pb = block_size(mode), perm_b(mode)
    out = bytearray()
    while len(text) >= bcs:
        for i in range(0, bcs, 8):
            w = int.from_bytes(text[i:i + 8], "big")
            o = s[i // 8] ^ w
            out += o.to_bytes(8, "big")
            s[i // 8] = o if enc else w
        perm(pb, s)
        text = text[bcs:]
    for i, b in enumerate(text):
        off = 56 - 8 * (i % 8)
        o = (s[i // 8] >> off & 0xFF) ^ b
        out.append(o)
        s[i // 8] = s[i // 8] & ~(0xFF << off) & M64 | (o if enc else b) << off
    s[len(text) // 8] ^= 0x80 << (56 - 8 * (len(text) % 8))
    return bytes(out)


def _finalize(mode, s, k):
    w = block_size(mode) // 8
    if mode == ASCON80PQ:
        s[w] ^= (k[0] << 32 | k[1] >> 32) & M64
        s[w + 1] ^= (k[1] << 32 | k[2] >> 32) & M64
        s[w + 2] ^= k[2] << 32 & M64
    else:
        s[w] ^= k[1]
        s[w + 1] ^= k[2]
    perm(PERM_A, s)
    return (s[3] ^ k[1]).to_bytes(8, "big") + (s[4] ^ k[2]).to_bytes(8, "big")


def seal(mode, key, nonce, pt, aad=b""):
    """Cipher.Seal: ciphertext || tag"""
    k = _key_words(mode, key)
    s = _initialize(mode, k, nonce)
    _assoc_data(mode, s, aad)
    ct = _proc_text(mode, s, pt, True)
    return ct + _finalize(mode, s, k)


def open(mode, key, nonce, ct, aad=b""):
    """Cipher.Open: the plaintext, or None where the tag does not verify (or ct is shorter than a tag)"""
    if len(ct) < TAG_SIZE:
        return None
    k = _key_words(mode, key)
    s = _initialize(mode, k, nonce)
    _assoc_data(mode, s, aad)
    pt = _proc_text(mode, s, ct[:-TAG_SIZE], False)
    return pt if _finalize(mode, s, k) == ct[-TAG_SIZE:] else None
