"""AES-128-GCM and AES-256-GCM in plain Python: the checker of the batch AEAD.  AES from FIPS 197 (a table S-box is fine here: this is
a test), GCM from NIST SP 800-38D with GHASH as big-integer arithmetic.  12-byte nonces and 16-byte tags only, as the library serves
them.  Sequence nonces as hpke/aead.go:47-52: base_nonce XOR BE96(seq)."""
NONCE_BYTES, TAG_BYTES = 12, 16
KEY_SIZES = (16, 32)


def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        x = inv[a]
        y = x
        for _ in range(4):
            x = ((x << 1) | (x >> 7)) & 0xFF
            y ^= x
        box.append(y ^ 0x63)
    return box


SBOX = _make_sbox()
_MUL2 = [_xtime(a) for a in range(256)]
_MUL3 = [_xtime(a) ^ a for a in range(256)]


def expand_key(key):
    """FIPS 197 5.2: the round keys as a list of 16-byte strings"""
    nk = len(key) // 4
    if len(key) not in KEY_SIZES:
        raise ValueError("AES-128 and AES-256 only")
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _xtime(rcon)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[x] for x in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(nr + 1)]


def encrypt_block(rk, block):
    """FIPS 197 5.1 on one 16-byte block; the state is column-major, as the bytes come"""
    s = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, len(rk)):
        s = [SBOX[x] for x in s]
        s = [s[(4 * c + r_ + 4 * r_) % 16] for c in range(4) for r_ in range(4)]      # ShiftRows: row r_ of column c from column c + r_
        if r != len(rk) - 1:
            t = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                t += [_MUL2[a[j]] ^ _MUL3[a[(j + 1) % 4]] ^ a[(j + 2) % 4] ^ a[(j + 3) % 4] for j in range(4)]
            s = t
        s = [a ^ b for a, b in zip(s, rk[r])]
    return bytes(s)


_R = 0xE1 << 120


def ghash_mul(x, y):
    """SP 800-38D 6.3 on integers whose most significant bit is the block's bit 0"""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


def ghash(h, aad, ct):
    """SP 800-38D 6.4 over aad padded || ct padded || the two bit lengths; the multiples h x^i are made once"""
    vs, v = [], h
    for _ in range(128):
        vs.append(v)
        v = (v >> 1) ^ _R if v & 1 else v >> 1

    def mul_h(x):
        z = 0
        for i in range(128):
            if (x >> (127 - i)) & 1:
                z ^= vs[i]
        return z

    y = 0
    for data in (aad, ct):
        for o in range(0, len(data), 16):
            y = mul_h(y ^ int.from_bytes(data[o:o + 16].ljust(16, b"\0"), "big"))
    return mul_h(y ^ (8 * len(aad) << 64 | 8 * len(ct)))


def _ctr(rk, nonce, data):
    out = bytearray()
    for o in range(0, len(data), 16):
        ks = encrypt_block(rk, nonce + ((2 + o // 16) & 0xFFFFFFFF).to_bytes(4, "big"))
        out += bytes(a ^ b for a, b in zip(data[o:o + 16], ks))
    return bytes(out)


def _tag(rk, nonce, aad, ct):
    h = int.from_bytes(encrypt_block(rk, bytes(16)), "big")
    ej0 = int.from_bytes(encrypt_block(rk, nonce + b"\0\0\0\1"), "big")
    return (ghash(h, aad, ct) ^ ej0).to_bytes(16, "big")


def seq_nonce(base_nonce, seq):
    return bytes(a ^ b for a, b in zip(base_nonce, seq.to_bytes(12, "big")))


def seal(key, nonce, pt, aad=b""):
    """ct || tag"""
    if len(nonce) != NONCE_BYTES:
        raise ValueError("12-byte nonces only")
    rk = expand_key(key)
    ct = _ctr(rk, nonce, pt)
    return ct + _tag(rk, nonce, aad, ct)


def open_(key, nonce, ct, aad=b""):
    """the plaintext, or None where the tag is wrong"""
    if len(nonce) != NONCE_BYTES or len(ct) < TAG_BYTES:
        raise ValueError("12-byte nonces and whole tags only")
    rk = expand_key(key)
    body, tag = ct[:-16], ct[-16:]
    diff = 0
    for a, b in zip(_tag(rk, nonce, aad, body), tag):
        diff |= a ^ b
    return None if diff else _ctr(rk, nonce, body)
