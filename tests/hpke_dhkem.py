"""HPKE DHKEM (RFC 9180 section 4.1) over X25519 / HKDF-SHA256 (KEM id 0x20) and X448 / HKDF-SHA512 (0x21) in plain Python,
written from the reference's hpke/kembase.go and hpke/xkem.go over hashlib, hmac and the ladders of tests/x25519.py and
tests/curve448.py.  The checker for the HPKE tests.  Test infrastructure only.

Every operation returns None where the reference returns an error (a Shared that reports a low-order point)."""
import hashlib
import hmac

import curve448
import x25519 as x255

X25519_SHA256, X448_SHA512 = 0x20, 0x21
VERSION = b"HPKE-v1"
P255 = 2**255 - 19
# dh/x25519/curve.go:71-96: the u-coordinates of order 1, 2, 4, 8 (0, 1, p - 1 and the two of order 8)
LOW_ORDER_255 = {0, 1, P255 - 1,
                 int.from_bytes(bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"), "little"),
                 int.from_bytes(bytes.fromhex("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157"), "little")}


class Kem:
    def __init__(self, kem_id):
        self.id = kem_id
        self.hash, self.N = {X25519_SHA256: (hashlib.sha256, 32), X448_SHA512: (hashlib.sha512, 56)}[kem_id]
        self.Nh = self.hash().digest_size        # kemBase.SharedKeySize
        self.suite = b"KEM" + kem_id.to_bytes(2, "big")

    # ---- kembase.go:52-82 ----
    def labeled_extract(self, salt, label, ikm):
        return hmac.new(salt or b"\0" * self.Nh, VERSION + self.suite + label + ikm, self.hash).digest()

    def labeled_expand(self, prk, label, info, length):
        assert length <= self.Nh  # one block of HKDF-Expand
        labeled = length.to_bytes(2, "big") + VERSION + self.suite + label + info
        return hmac.new(prk, labeled + b"\x01", self.hash).digest()[:length]

    def extract_expand(self, dh, kem_ctx):
        return self.labeled_expand(self.labeled_extract(b"", b"eae_prk", dh), b"shared_secret", kem_ctx, self.Nh)

    # ---- xkem.go ----
    def public(self, sk):
        return x255.public(sk) if self.N == 32 else curve448.x448(sk)[0]

    def dh(self, sk, pk):
        """calcDH: None where x25519.Shared / x448.Shared return false"""
        if self.N == 32:
            if (int.from_bytes(pk, "little") & (2**255 - 1)) % P255 in LOW_ORDER_255:
                return None
            return x255.x25519(sk, pk)
        out, ok = curve448.x448(sk, pk)
        return out if ok else None

    def derive_keypair(self, ikm):
        """-> (sk, pk); sk is the raw Expand output"""
        sk = self.labeled_expand(self.labeled_extract(b"", b"dkp_prk", ikm), b"sk", b"", self.N)
        return sk, self.public(sk)

    # ---- kembase.go:120-241 ----
    def encap(self, pkR, ikmE):
        skE, enc = self.derive_keypair(ikmE)
        dh = self.dh(skE, pkR)
        if dh is None:
            return None
        return enc, self.extract_expand(dh, enc + pkR)

    def decap(self, skR, enc, pkR=None):
        dh = self.dh(skR, enc)
        if dh is None:
            return None
        return self.extract_expand(dh, enc + (self.public(skR) if pkR is None else pkR))

    def auth_encap(self, pkR, skS, ikmE, pkS=None):
        skE, enc = self.derive_keypair(ikmE)
        dh1, dh2 = self.dh(skE, pkR), self.dh(skS, pkR)
        if dh1 is None or dh2 is None:
            return None
        return enc, self.extract_expand(dh1 + dh2, enc + pkR + (self.public(skS) if pkS is None else pkS))

    def auth_decap(self, skR, enc, pkS, pkR=None):
        dh1, dh2 = self.dh(skR, enc), self.dh(skR, pkS)
        if dh1 is None or dh2 is None:
            return None
        return self.extract_expand(dh1 + dh2, enc + (self.public(skR) if pkR is None else pkR) + pkS)


def low_order_points(kem_id):
    """public keys that Shared rejects, as N-byte rows (the aliases above p included)"""
    if kem_id == X25519_SHA256:
        vals = sorted(LOW_ORDER_255) + [P255, P255 + 1]
        return [v.to_bytes(32, "little") for v in vals]
    p = curve448.P
    return [v.to_bytes(56, "little") for v in (0, 1, p - 1, p, p + 1)]
