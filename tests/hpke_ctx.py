"""HPKE contexts (RFC 9180 sections 5 and 6) in plain Python: the key schedule, ChaCha20-Poly1305 Seal / Open and Export, written
from the reference's hpke/util.go, hpke/aead.go and hpke/hpke.go and from RFC 8439, over hashlib, hmac and tests/hpke_dhkem.py.
Poly1305 is big-integer arithmetic.  The checker for the HPKE context tests.  Test infrastructure only.

Every operation returns None where the reference returns an error."""
import hashlib
import hmac
import struct

import hpke_dhkem as hp

KDF_SHA256, KDF_SHA512 = 1, 3
AEAD_CHACHA20POLY1305, AEAD_EXPORT_ONLY = 3, 0xFFFF
MODE_BASE, MODE_PSK, MODE_AUTH, MODE_AUTH_PSK = range(4)
HASHES = {KDF_SHA256: hashlib.sha256, KDF_SHA512: hashlib.sha512}


# ---- RFC 8439 ----
def _rotl(v, c):
    return ((v << c) & 0xffffffff) | (v >> (32 - c))


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key, counter, nonce):
    init = list(struct.unpack("<4I", b"expand 32-byte k") + struct.unpack("<8I", key) + (counter,) + struct.unpack("<3I", nonce))
    x = list(init)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & 0xffffffff for a, b in zip(x, init)))


def chacha20_xor(key, counter, nonce, data):
    out = bytearray()
    for i in range(0, len(data), 64):
        ks = chacha20_block(key, counter + i // 64, nonce)
        out += bytes(a ^ b for a, b in zip(data[i:i + 64], ks))
    return bytes(out)


def poly1305(key, msg):
    """key = r || s (32 bytes); r is clamped here"""
    r = int.from_bytes(key[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    s = int.from_bytes(key[16:], "little")
    p, h = 2**130 - 5, 0
    for i in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % p
    return ((h + s) % 2**128).to_bytes(16, "little")


def _pad16(b):
    return b + bytes(-len(b) % 16)


def _tag(key, nonce, aad, ct):
    return poly1305(chacha20_block(key, 0, nonce)[:32], _pad16(aad) + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct)))


def aead_seal(key, nonce, pt, aad):
    ct = chacha20_xor(key, 1, nonce, pt)
    return ct + _tag(key, nonce, aad, ct)


def aead_open(key, nonce, ct, aad):
    if len(ct) < 16 or not hmac.compare_digest(_tag(key, nonce, aad, ct[:-16]), ct[-16:]):
        return None
    return chacha20_xor(key, 1, nonce, ct[:-16])


# ---- hpke/util.go, hpke/aead.go, hpke/hpke.go ----
class Suite:
    def __init__(self, kem, kdf, aead):
        self.kem_id, self.kdf_id, self.aead_id = kem, kdf, aead
        self.kem, self.hash = hp.Kem(kem), HASHES[kdf]
        self.Nh = self.hash().digest_size
        self.id = b"HPKE" + struct.pack(">HHH", kem, kdf, aead)        # util.go:85-91

    def labeled_extract(self, salt, label, ikm):
        return hmac.new(salt or bytes(self.Nh), hp.VERSION + self.id + label + ikm, self.hash).digest()

    def labeled_expand(self, prk, label, info, length):
        assert 0 < length <= 255 * self.Nh
        labeled = struct.pack(">H", length) + hp.VERSION + self.id + label + info
        out, t, i = b"", b"", 1
        while len(out) < length:
            t = hmac.new(prk, t + labeled + bytes([i]), self.hash).digest()
            out, i = out + t, i + 1
        return out[:length]

    def key_schedule(self, mode, ss, info, psk=b"", psk_id=b""):
        """-> dict(key_schedule_context, secret, key, base_nonce, exporter_secret) or None (verifyPSKInputs)"""
        if bool(psk) != bool(psk_id) or bool(psk) != (mode in (MODE_PSK, MODE_AUTH_PSK)):
            return None
        ksc = bytes([mode]) + self.labeled_extract(b"", b"psk_id_hash", psk_id) + self.labeled_extract(b"", b"info_hash", info)
        secret = self.labeled_extract(ss, b"secret", psk)
        seal = self.aead_id != AEAD_EXPORT_ONLY
        return dict(key_schedule_context=ksc, secret=secret,
                    key=self.labeled_expand(secret, b"key", ksc, 32) if seal else b"",
                    base_nonce=self.labeled_expand(secret, b"base_nonce", ksc, 12) if seal else b"",
                    exporter_secret=self.labeled_expand(secret, b"exp", ksc, self.Nh))

    def context_row(self, ks):
        """the library's context row: key[32] || base_nonce[12] || 0[4] || exporter_secret[Nh]"""
        return ks["key"].ljust(32, b"\0") + ks["base_nonce"].ljust(12, b"\0") + bytes(4) + ks["exporter_secret"]

    def setup_sender(self, mode, pkR, ikmE, info, psk=b"", psk_id=b"", skS=None):
        """-> (enc, key schedule dict) or None"""
        r = self.kem.auth_encap(pkR, skS, ikmE) if mode in (MODE_AUTH, MODE_AUTH_PSK) else self.kem.encap(pkR, ikmE)
        ks = r and self.key_schedule(mode, r[1], info, psk, psk_id)
        return (r[0], ks) if ks else None

    def setup_receiver(self, mode, skR, enc, info, psk=b"", psk_id=b"", pkS=None):
        ss = self.kem.auth_decap(skR, enc, pkS) if mode in (MODE_AUTH, MODE_AUTH_PSK) else self.kem.decap(skR, enc)
        return ss and self.key_schedule(mode, ss, info, psk, psk_id)

    @staticmethod
    def nonce(ks, seq):
        return (int.from_bytes(ks["base_nonce"], "big") ^ seq).to_bytes(12, "big")   # aead.go:47-52

    def seal(self, ks, seq, pt, aad):
        return aead_seal(ks["key"], self.nonce(ks, seq), pt, aad)

    def open(self, ks, seq, ct, aad):
        return aead_open(ks["key"], self.nonce(ks, seq), ct, aad)

    def export(self, ks, exporter_context, length):
        return self.labeled_expand(ks["exporter_secret"], b"sec", exporter_context, length)
