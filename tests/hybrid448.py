"""Kyber768-X448 and Kyber1024-X448 in plain Python: the checker for the X448 hybrids (the product side runs on the GPU).  Written
from kem/hybrid/hybrid.go (scheme{name, first, second}: :83-93, sizes :123-157, DeriveKeyPair :237-252,
EncapsulateDeterministically :273-301, Decapsulate :303-323) and kem/hybrid/xkem.go (X448 as a KEM: DeriveKeyPair :112-123,
X :134-158, EncapsulateDeterministically :160-178, Decapsulate :180-196) over hashlib's shake_256, the RFC 7748 ladder of
tests/curve448.py and the oracle's round-3 Kyber.  Test infrastructure only."""
import hashlib

import numpy as np

import curve448
from oracle import orc

KYBER768_X448, KYBER1024_X448 = 5, 6
NAMES = {KYBER768_X448: "Kyber768-X448", KYBER1024_X448: "Kyber1024-X448"}
PARAM = {KYBER768_X448: 768, KYBER1024_X448: 1024}
X = 56  # x448.Size: the X448 KEM's seed, encapsulation seed, keys, ciphertext and shared secret


def sizes(scheme):
    ek, dk, ct = orc.KEM_SIZES[PARAM[scheme]]
    return dict(seed=max(X, 64), eseed=max(X, 32), pk=X + ek, sk=X + dk, ct=X + ct, ss=X + 32)


def _shake(data: bytes, n: int) -> bytes:
    return hashlib.shake_256(data).digest(n)


def _rows(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width).copy()


def x_derive(seed: bytes):
    """xScheme.DeriveKeyPair: sk = SHAKE256(seed)[:56], pk = X448(sk, 5)"""
    sk = _shake(seed, X)
    return curve448.x448(sk)[0], sk


def keygen(scheme, seeds):
    """DeriveKeyPair for every 64-byte seed -> (pk, sk): SHAKE256(seed) -> 56 bytes for X448 (first), then 64 for Kyber"""
    param = PARAM[scheme]
    ex = [_shake(bytes(s), X + 64) for s in seeds]
    xk = [x_derive(e[:X]) for e in ex]
    ek, dk = orc.kyber_r3_keygen(param, _rows([e[X:] for e in ex], 64))
    pk = np.concatenate([_rows([p for p, _ in xk], X), ek], axis=1)
    sk = np.concatenate([_rows([s for _, s in xk], X), dk], axis=1)
    return pk, sk


def encaps(scheme, pk, eseeds):
    """EncapsulateDeterministically -> (ct, ss, status): status 1 and all-zero rows where x448.Shared refuses pk_X (nil, nil, err)"""
    param = PARAM[scheme]
    n = len(pk)
    ex = [_shake(bytes(s), X + 32) for s in eseeds]
    ct_x, ss_x, status = [], [], np.zeros(n, np.uint8)
    for i in range(n):
        pk2, sk2 = x_derive(ex[i][:X])
        ss, ok = curve448.x448(sk2, bytes(pk[i, :X]))
        status[i] = 0 if ok else 1
        ct_x.append(pk2)
        ss_x.append(ss)
    ct_k, ss_k = orc.kyber_r3_encaps(param, pk[:, X:].copy(), _rows([e[X:] for e in ex], 32))
    ct = np.concatenate([_rows(ct_x, X), ct_k], axis=1)
    ss = np.concatenate([_rows(ss_x, X), ss_k], axis=1)
    ct[status != 0] = 0
    ss[status != 0] = 0
    return ct, ss, status


def decaps(scheme, sk, ct):
    """Decapsulate -> (ss, status): status 1 and a zero row where x448.Shared refuses ct_X"""
    param = PARAM[scheme]
    n = len(sk)
    ss_x, status = [], np.zeros(n, np.uint8)
    for i in range(n):
        ss, ok = curve448.x448(bytes(sk[i, :X]), bytes(ct[i, :X]))
        status[i] = 0 if ok else 1
        ss_x.append(ss)
    ss_k = orc.kyber_r3_decaps(param, sk[:, X:].copy(), ct[:, X:].copy())
    ss = np.concatenate([_rows(ss_x, X), ss_k], axis=1)
    ss[status != 0] = 0
    return ss, status
