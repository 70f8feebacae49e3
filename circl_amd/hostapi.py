"""Host-buffer (numpy) wrappers over the C ABI -- what the cgo bridge would call."""
import ctypes as C

import numpy as np

from . import _native as nat

KEM_SIZES = {512: (800, 1632, 768), 768: (1184, 2400, 1088), 1024: (1568, 3168, 1568)}  # ek, dk, ct
# pk, sig; 2 / 3 / 5 = round-3 Dilithium2/3/5 (sign/dilithium/mode{2,3,5}): no context, deterministic, 32-byte tr and c~
DSA_SIZES = {44: (1312, 2420), 65: (1952, 3309), 87: (2592, 4627), 2: (1312, 2420), 3: (1952, 3293), 5: (2592, 4595)}
DSA_SK_SIZES = {44: 2560, 65: 4032, 87: 4896, 2: 2528, 3: 4000, 5: 4864}


def _u8(x, cols):
    a = np.ascontiguousarray(np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)
    return a.reshape(-1, cols)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return nat.lib().circl_hip_device_count()


def mlkem_encaps(param, ek, m, device=0):
    EK, _, CT = KEM_SIZES[param]
    ek, m = _u8(ek, EK), _u8(m, 32)
    n = len(ek)
    assert len(m) == n
    ct = np.empty((n, CT), np.uint8)
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_encaps(param, _p(ek), _p(m), _p(ct), _p(ss), _p(st), n, device), "mlkem_encaps")
    return ct, ss, st


def mlkem_decaps(param, dk, ct, device=0):
    _, DK, CT = KEM_SIZES[param]
    dk, ct = _u8(dk, DK), _u8(ct, CT)
    n = len(dk)
    assert len(ct) == n
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_decaps(param, _p(dk), _p(ct), _p(ss), _p(st), n, device), "mlkem_decaps")
    return ss, st


def mlkem_keygen(param, seeds, device=0):
    EK, DK, _ = KEM_SIZES[param]
    seeds = _u8(seeds, 64)
    n = len(seeds)
    ek = np.empty((n, EK), np.uint8)
    dk = np.empty((n, DK), np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_keygen(param, _p(seeds), _p(ek), _p(dk), n, device), "mlkem_keygen")
    return ek, dk


def mlkem_encaps_shared(param, ek, m, device=0):
    """one key for the whole batch -> ct, ss, status"""
    EK, _, CT = KEM_SIZES[param]
    ek, m = _u8(ek, EK), _u8(m, 32)
    assert len(ek) == 1
    n = len(m)
    ct = np.empty((n, CT), np.uint8)
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_encaps_shared(param, _p(ek), _p(m), _p(ct), _p(ss), _p(st), n, device), "mlkem_encaps_shared")
    return ct, ss, st


def mlkem_decaps_shared(param, dk, ct, device=0):
    """one private key for the whole batch -> ss, status"""
    _, DK, CT = KEM_SIZES[param]
    dk, ct = _u8(dk, DK), _u8(ct, CT)
    assert len(dk) == 1
    n = len(ct)
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_decaps_shared(param, _p(dk), _p(ct), _p(ss), _p(st), n, device), "mlkem_decaps_shared")
    return ss, st


def _idx(key_idx, n):
    a = np.ascontiguousarray(key_idx, dtype=np.uint32).reshape(-1)
    assert len(a) == n
    return a


def mlkem_encaps_keyed(param, ek_table, key_idx, m, device=0):
    """item i encapsulates to row key_idx[i] of ek_table -> ct, ss, status"""
    EK, _, CT = KEM_SIZES[param]
    ek_table, m = _u8(ek_table, EK), _u8(m, 32)
    n = len(m)
    idx = _idx(key_idx, n)
    ct = np.empty((n, CT), np.uint8)
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_encaps_keyed(param, _p(ek_table), len(ek_table), _p(idx), _p(m), _p(ct), _p(ss), _p(st), n, device),
              "mlkem_encaps_keyed")
    return ct, ss, st


def mlkem_decaps_keyed(param, dk_table, key_idx, ct, device=0):
    """item i is decapsulated with row key_idx[i] of dk_table -> ss, status"""
    _, DK, CT = KEM_SIZES[param]
    dk_table, ct = _u8(dk_table, DK), _u8(ct, CT)
    n = len(ct)
    idx = _idx(key_idx, n)
    ss = np.empty((n, 32), np.uint8)
    st = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_decaps_keyed(param, _p(dk_table), len(dk_table), _p(idx), _p(ct), _p(ss), _p(st), n, device),
              "mlkem_decaps_keyed")
    return ss, st


# round-3 Kyber (kem/kyber/kyber{512,768,1024}): no per-item failures
def kyber_keygen(param, seeds, device=0):
    EK, DK, _ = KEM_SIZES[param]
    seeds = _u8(seeds, 64)
    n = len(seeds)
    ek = np.empty((n, EK), np.uint8)
    dk = np.empty((n, DK), np.uint8)
    nat.check(nat.lib().circl_hip_kyber_keygen(param, _p(seeds), _p(ek), _p(dk), n, device), "kyber_keygen")
    return ek, dk


def kyber_encaps(param, ek, seeds, device=0):
    EK, _, CT = KEM_SIZES[param]
    ek, seeds = _u8(ek, EK), _u8(seeds, 32)
    n = len(ek)
    assert len(seeds) == n
    ct = np.empty((n, CT), np.uint8)
    ss = np.empty((n, 32), np.uint8)
    nat.check(nat.lib().circl_hip_kyber_encaps(param, _p(ek), _p(seeds), _p(ct), _p(ss), n, device), "kyber_encaps")
    return ct, ss


def kyber_decaps(param, dk, ct, device=0):
    _, DK, CT = KEM_SIZES[param]
    dk, ct = _u8(dk, DK), _u8(ct, CT)
    n = len(dk)
    assert len(ct) == n
    ss = np.empty((n, 32), np.uint8)
    nat.check(nat.lib().circl_hip_kyber_decaps(param, _p(dk), _p(ct), _p(ss), n, device), "kyber_decaps")
    return ss


def _blob(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if len(items):
        off[1:] = np.cumsum([len(x) for x in items])
    blob = np.frombuffer(b"".join(bytes(x) for x in items) + b"\0" * 16, dtype=np.uint8).copy()
    return blob, off


def mldsa_keygen(param, seeds, device=0):
    PK, _ = DSA_SIZES[param]
    SK = DSA_SK_SIZES[param]
    seeds = _u8(seeds, 32)
    n = len(seeds)
    pk = np.empty((n, PK), np.uint8)
    sk = np.empty((n, SK), np.uint8)
    nat.check(nat.lib().circl_hip_mldsa_keygen(param, _p(seeds), _p(pk), _p(sk), n, device), "mldsa_keygen")
    return pk, sk


def mldsa_sign(param, sk, msgs, ctxs=None, rnd=None, internal=False, device=0):
    """deterministic when rnd is None"""
    _, SIG = DSA_SIZES[param]
    SK = DSA_SK_SIZES[param]
    sk = _u8(sk, SK)
    n = len(sk)
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    sig = np.empty((n, SIG), np.uint8)
    r = None if rnd is None else _p(_u8(rnd, 32))
    if internal:
        rc = nat.lib().circl_hip_mldsa_sign_internal(param, _p(sk), _p(mb), _p(mo), r, _p(sig), n, device)
    elif ctxs is None:
        rc = nat.lib().circl_hip_mldsa_sign(param, _p(sk), _p(mb), _p(mo), None, None, r, _p(sig), n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_mldsa_sign(param, _p(sk), _p(mb), _p(mo), _p(cb), _p(co), r, _p(sig), n, device)
    nat.check(rc, "mldsa_sign")
    return sig


def mldsa_sign_shared(param, sk, msgs, ctxs=None, rnd=None, device=0):
    """n messages signed with ONE private key -> (n, SIG)"""
    _, SIG = DSA_SIZES[param]
    sk = _u8(sk, DSA_SK_SIZES[param])
    assert len(sk) == 1
    n = len(msgs)
    mb, mo = _blob(msgs)
    sig = np.empty((n, SIG), np.uint8)
    r = None if rnd is None else _p(_u8(rnd, 32))
    if ctxs is None:
        rc = nat.lib().circl_hip_mldsa_sign_shared(param, _p(sk), _p(mb), _p(mo), None, None, r, _p(sig), n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_mldsa_sign_shared(param, _p(sk), _p(mb), _p(mo), _p(cb), _p(co), r, _p(sig), n, device)
    nat.check(rc, "mldsa_sign_shared")
    return sig


def mldsa_verify_internal(param, pk, sig, msgs, device=0):
    PK, SIG = DSA_SIZES[param]
    pk, sig = _u8(pk, PK), _u8(sig, SIG)
    n = len(pk)
    mb, mo = _blob(msgs)
    ok = np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_mldsa_verify_internal(param, _p(pk), _p(sig), _p(mb), _p(mo), _p(ok), n, device), "mldsa_verify_internal")
    return ok


def mldsa_verify(param, pk, sig, msgs, ctxs=None, device=0):
    PK, SIG = DSA_SIZES[param]
    pk, sig = _u8(pk, PK), _u8(sig, SIG)
    n = len(pk)
    assert len(sig) == n and len(msgs) == n
    mb, mo = _blob(msgs)
    ok = np.empty(n, np.uint8)
    if ctxs is None:
        rc = nat.lib().circl_hip_mldsa_verify(param, _p(pk), _p(sig), _p(mb), _p(mo), None, None, _p(ok), n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_mldsa_verify(param, _p(pk), _p(sig), _p(mb), _p(mo), _p(cb), _p(co), _p(ok), n, device)
    nat.check(rc, "mldsa_verify")
    return ok


def mldsa_verify_shared(param, pk, sig, msgs, ctxs=None, device=0):
    """n signatures under ONE public key -> ok (n,)"""
    PK, SIG = DSA_SIZES[param]
    pk, sig = _u8(pk, PK), _u8(sig, SIG)
    assert len(pk) == 1
    n = len(sig)
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    ok = np.empty(n, np.uint8)
    if ctxs is None:
        rc = nat.lib().circl_hip_mldsa_verify_shared(param, _p(pk), _p(sig), _p(mb), _p(mo), None, None, _p(ok), n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_mldsa_verify_shared(param, _p(pk), _p(sig), _p(mb), _p(mo), _p(cb), _p(co), _p(ok), n, device)
    nat.check(rc, "mldsa_verify_shared")
    return ok


def mldsa_verify_keyed(param, pk_table, key_idx, sig, msgs, ctxs=None, device=0):
    """signature i is checked under row key_idx[i] of pk_table -> ok (n,)"""
    PK, SIG = DSA_SIZES[param]
    pk_table, sig = _u8(pk_table, PK), _u8(sig, SIG)
    n = len(sig)
    assert len(msgs) == n
    idx = _idx(key_idx, n)
    mb, mo = _blob(msgs)
    ok = np.empty(n, np.uint8)
    if ctxs is None:
        rc = nat.lib().circl_hip_mldsa_verify_keyed(param, _p(pk_table), len(pk_table), _p(idx), _p(sig), _p(mb), _p(mo), None, None, _p(ok), n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_mldsa_verify_keyed(param, _p(pk_table), len(pk_table), _p(idx), _p(sig), _p(mb), _p(mo), _p(cb), _p(co), _p(ok), n, device)
    nat.check(rc, "mldsa_verify_keyed")
    return ok


class KeyTable:
    """A parsed-key cache that lives across calls (circl_hip_*_keytable_new): the counterpart of CIRCL's key objects, which keep
    A^T / H(ek) (ML-KEM) or A / tr (ML-DSA) after unmarshalling.  kind: "mlkem-public", "mlkem-private", "mldsa-public", "mldsa-private",
    "hybrid-public", "hybrid-private" (param = the hybrid scheme id).  device = -1: replicated on every device, calls shard the batch."""

    def __init__(self, kind, param, keys, device=0):
        import ctypes as C
        self.kind, self.param, self.device = kind, param, device
        self.handle = C.c_void_p()
        self.key_status = None
        L = nat.lib()
        if kind.startswith("mlkem"):
            EK, DK, _ = KEM_SIZES[param]
            priv = kind == "mlkem-private"
            keys = _u8(keys, DK if priv else EK)
            self.nkeys = len(keys)
            self.key_status = np.zeros(self.nkeys, np.uint8)
            nat.check(L.circl_hip_mlkem_keytable_new(param, 1 if priv else 0, _p(keys), self.nkeys, device, _p(self.key_status), C.byref(self.handle)),
                      "mlkem_keytable_new")
        elif kind == "mldsa-private":
            keys = _u8(keys, nat.lib().circl_hip_mldsa_sk_size(param))
            self.nkeys = len(keys)
            nat.check(L.circl_hip_mldsa_privkeys_new(param, _p(keys), self.nkeys, device, C.byref(self.handle)), "mldsa_privkeys_new")
        elif kind.startswith("hybrid"):  # param = the hybrid scheme id (XWING, X25519MLKEM768)
            priv = kind == "hybrid-private"
            keys = _u8(keys, HYBRID_SIZES[param]["sk" if priv else "pk"])
            self.nkeys = len(keys)
            self.key_status = np.zeros(self.nkeys, np.uint8)
            nat.check(L.circl_hip_hybrid_keytable_new(param, 1 if priv else 0, _p(keys), self.nkeys, device, _p(self.key_status), C.byref(self.handle)),
                      "hybrid_keytable_new")
        else:
            PK, _ = DSA_SIZES[param]
            keys = _u8(keys, PK)
            self.nkeys = len(keys)
            nat.check(L.circl_hip_mldsa_keytable_new(param, _p(keys), self.nkeys, device, C.byref(self.handle)), "mldsa_keytable_new")

    def close(self):
        if self.handle:
            nat.lib().circl_hip_keytable_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_coalesce(self, max_items, max_wait_us=0):
        """circl_hip_keytable_set_coalesce: small calls of concurrent callers through this table share launches (0 = off)"""
        nat.check(nat.lib().circl_hip_keytable_set_coalesce(self.handle, max_items, max_wait_us), "keytable_set_coalesce")

    # ---- the asynchronous form (circl_hip_keytable_async_start / *_table_submit / circl_hip_poll / circl_hip_wait) ----
    def async_start(self, max_items, max_wait_us=0, eventfd=False):
        nat.check(nat.lib().circl_hip_keytable_async_start(self.handle, max_items, max_wait_us, 1 if eventfd else 0), "keytable_async_start")

    def async_stop(self):
        """CIRCL_HIP_OK, or CIRCL_HIP_EBUSY (returned, not raised) while calls are inside the table"""
        return nat.lib().circl_hip_keytable_async_stop(self.handle)

    def eventfd(self, replica=0):
        return nat.lib().circl_hip_keytable_eventfd(self.handle, replica)

    def submit_encaps(self, m, ct, ss, st, key_idx=None):
        """Returns (rc, ticket); the output arrays (caller-owned, C-contiguous uint8) are filled once the ticket is done."""
        import ctypes as C
        m = _u8(m, 32)
        n = len(m)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_mlkem_encaps_table_submit(self.handle, self._kidx(key_idx, n), _p(m), _p(ct), _p(ss), _p(st), n, C.byref(t))
        return rc, t.value

    def submit_decaps(self, ct, ss, st, key_idx=None):
        import ctypes as C
        _, _, CT = KEM_SIZES[self.param]
        ct = _u8(ct, CT)
        n = len(ct)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_mlkem_decaps_table_submit(self.handle, self._kidx(key_idx, n), _p(ct), _p(ss), _p(st), n, C.byref(t))
        return rc, t.value

    def submit_hybrid_encaps(self, eseeds, ct, ss, st, key_idx=None):
        import ctypes as C
        es = _u8(eseeds, HYBRID_SIZES[self.param]["eseed"])
        n = len(es)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_hybrid_encaps_table_submit(self.handle, self._kidx(key_idx, n), _p(es), _p(ct), _p(ss), _p(st), n, C.byref(t))
        return rc, t.value

    def submit_hybrid_decaps(self, ct_in, ss, st, key_idx=None):
        import ctypes as C
        c = _u8(ct_in, HYBRID_SIZES[self.param]["ct"])
        n = len(c)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_hybrid_decaps_table_submit(self.handle, self._kidx(key_idx, n), _p(c), _p(ss), _p(st), n, C.byref(t))
        return rc, t.value

    def submit_verify(self, sigs, msgs, ok, ctxs=None, key_idx=None):
        import ctypes as C
        _, SIG = DSA_SIZES[self.param]
        sigs = _u8(sigs, SIG)
        n = len(sigs)
        mb, mo = _blob(msgs)
        cb, cofs = _blob(ctxs) if ctxs is not None else (None, None)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_mldsa_verify_table_submit(self.handle, self._kidx(key_idx, n), _p(sigs), _p(mb), _p(mo), _p(cb) if cb is not None else None,
                                                           _p(cofs) if cofs is not None else None, _p(ok), n, C.byref(t))
        return rc, t.value

    def poll(self, tickets):
        """-> list of states (1 done, 0 pending, < 0 failed)"""
        t = np.asarray(tickets, np.uint64)
        st = np.zeros(len(t), np.int8)
        nat.lib().circl_hip_poll(self.handle, _p(t), len(t), _p(st))
        return [int(x) for x in st]

    def wait(self, ticket, timeout_us=-1):
        return nat.lib().circl_hip_wait(self.handle, int(ticket), int(timeout_us))

    def try_close(self):
        """circl_hip_keytable_close: 0 and the table is gone, or CIRCL_HIP_EBUSY"""
        rc = nat.lib().circl_hip_keytable_close(self.handle)
        if rc == 0:
            self.handle = None
        return rc

    def coalesce_stats(self):
        """(calls, items, launches) that went through the table's coalescer"""
        import ctypes as C
        c, i, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        nat.check(nat.lib().circl_hip_keytable_coalesce_stats(self.handle, C.byref(c), C.byref(i), C.byref(l)), "keytable_coalesce_stats")
        return c.value, i.value, l.value

    def _kidx(self, key_idx, n):
        return None if key_idx is None else _p(_idx(key_idx, n))

    def encaps(self, m, key_idx=None):
        """item i encapsulates to entry key_idx[i] (None: entry 0) -> ct, ss, status"""
        _, _, CT = KEM_SIZES[self.param]
        m = _u8(m, 32)
        n = len(m)
        ct, ss, st = np.empty((n, CT), np.uint8), np.empty((n, 32), np.uint8), np.empty(n, np.uint8)
        nat.check(nat.lib().circl_hip_mlkem_encaps_table(self.handle, self._kidx(key_idx, n), _p(m), _p(ct), _p(ss), _p(st), n), "mlkem_encaps_table")
        return ct, ss, st

    def decaps(self, ct, key_idx=None):
        _, _, CT = KEM_SIZES[self.param]
        ct = _u8(ct, CT)
        n = len(ct)
        ss, st = np.empty((n, 32), np.uint8), np.empty(n, np.uint8)
        nat.check(nat.lib().circl_hip_mlkem_decaps_table(self.handle, self._kidx(key_idx, n), _p(ct), _p(ss), _p(st), n), "mlkem_decaps_table")
        return ss, st

    def sign(self, msgs, ctxs=None, rnd=None, key_idx=None):
        """scheme.Sign with the prepared private key(s): message i with entry key_idx[i] (None: entry 0) -> (n, SIG)"""
        _, SIG = DSA_SIZES[self.param]
        n = len(msgs)
        mb, mo = _blob(msgs)
        sig = np.empty((n, SIG), np.uint8)
        cb, co = _blob(ctxs) if ctxs is not None else (None, None)
        r = None if rnd is None else _u8(rnd, 32)
        if key_idx is None:
            rc = nat.lib().circl_hip_mldsa_sign_table(self.handle, _p(mb), _p(mo), _p(cb) if ctxs is not None else None, _p(co) if ctxs is not None else None,
                                                      None if r is None else _p(r), _p(sig), n)
        else:
            rc = nat.lib().circl_hip_mldsa_sign_table_keyed(self.handle, self._kidx(key_idx, n), _p(mb), _p(mo), _p(cb) if ctxs is not None else None,
                                                            _p(co) if ctxs is not None else None, None if r is None else _p(r), _p(sig), n)
        nat.check(rc, "mldsa_sign_table")
        return sig

    def hybrid_encaps(self, eseeds, key_idx=None):
        S = HYBRID_SIZES[self.param]
        es = _u8(eseeds, S["eseed"])
        n = len(es)
        ct, ss, st = np.empty((n, S["ct"]), np.uint8), np.empty((n, S["ss"]), np.uint8), np.empty(n, np.uint8)
        nat.check(nat.lib().circl_hip_hybrid_encaps_table(self.handle, self._kidx(key_idx, n), _p(es), _p(ct), _p(ss), _p(st), n), "hybrid_encaps_table")
        return ct, ss, st

    def hybrid_decaps(self, ct, key_idx=None):
        S = HYBRID_SIZES[self.param]
        ct = _u8(ct, S["ct"])
        n = len(ct)
        ss, st = np.empty((n, S["ss"]), np.uint8), np.empty(n, np.uint8)
        nat.check(nat.lib().circl_hip_hybrid_decaps_table(self.handle, self._kidx(key_idx, n), _p(ct), _p(ss), _p(st), n), "hybrid_decaps_table")
        return ss, st

    def verify(self, sig, msgs, ctxs=None, key_idx=None):
        _, SIG = DSA_SIZES[self.param]
        sig = _u8(sig, SIG)
        n = len(sig)
        assert len(msgs) == n
        mb, mo = _blob(msgs)
        ok = np.empty(n, np.uint8)
        cb, co = _blob(ctxs) if ctxs is not None else (None, None)
        rc = nat.lib().circl_hip_mldsa_verify_table(self.handle, self._kidx(key_idx, n), _p(sig), _p(mb), _p(mo), _p(cb) if ctxs is not None else None,
                                                    _p(co) if ctxs is not None else None, _p(ok), n)
        nat.check(rc, "mldsa_verify_table")
        return ok


def mlkem_public_from_private(param, dk):
    """PrivateKey.Public() over a batch (kem/mlkem/mlkem768/kyber.go:323-328)"""
    EK, DK, _ = KEM_SIZES[param]
    dk = _u8(dk, DK)
    ek = np.empty((len(dk), EK), np.uint8)
    nat.check(nat.lib().circl_hip_mlkem_public_from_private(param, _p(dk), _p(ek), len(dk)), "mlkem_public_from_private")
    return ek


def mldsa_public_from_private(param, sk, device=0):
    """PrivateKey.Public() over a batch (sign/mldsa/mldsa65/internal/dilithium.go:473-484)"""
    sk = _u8(sk, nat.lib().circl_hip_mldsa_sk_size(param))
    pk = np.empty((len(sk), nat.lib().circl_hip_mldsa_pk_size(param)), np.uint8)
    nat.check(nat.lib().circl_hip_mldsa_public_from_private(param, _p(sk), _p(pk), len(sk), device), "mldsa_public_from_private")
    return pk


def keccak_f1600(states, rounds=24, device=0):
    a = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25).copy()
    nat.check(nat.lib().circl_hip_keccak_f1600(_p(a), len(a), rounds, device), "keccak_f1600")
    return a


def keccak_f1600_coop(states, device=0):
    a = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25).copy()
    nat.check(nat.lib().circl_hip_keccak_f1600_coop(_p(a), len(a), device), "keccak_f1600_coop")
    return a


def keccak_f1600_split(states, device=0):
    a = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25).copy()
    nat.check(nat.lib().circl_hip_keccak_f1600_split(_p(a), len(a), device), "keccak_f1600_split")
    return a


def mldsa_sample_in_ball(param, ctilde, sequential=False, device=0):
    """c~ rows -> (n, 256) uint32 challenge polynomials (PolyDeriveUniformBall)"""
    ct = {44: 32, 65: 48, 87: 64, 2: 32, 3: 32, 5: 32}[param]
    c = _u8(ctilde, ct)
    out = np.empty((len(c), 256), np.uint32)
    nat.check(nat.lib().circl_hip_mldsa_sample_in_ball(param, _p(c), _p(out), len(c), int(sequential), device), "mldsa_sample_in_ball")
    return out


def kyber_ntt(polys, inverse=False, device=0):
    a = np.ascontiguousarray(polys, dtype=np.int16).reshape(-1, 256).copy()
    nat.check(nat.lib().circl_hip_kyber_ntt(_p(a), len(a), int(inverse), device), "kyber_ntt")
    return a


def kyber_mulhat(a, b, device=0):
    a = np.ascontiguousarray(a, dtype=np.int16).reshape(-1, 256)
    b = np.ascontiguousarray(b, dtype=np.int16).reshape(-1, 256)
    out = np.empty_like(a)
    nat.check(nat.lib().circl_hip_kyber_mulhat(_p(out), _p(a), _p(b), len(a), device), "kyber_mulhat")
    return out


def dilithium_ntt(polys, inverse=False, device=0):
    a = np.ascontiguousarray(polys, dtype=np.uint32).reshape(-1, 256).copy()
    nat.check(nat.lib().circl_hip_dilithium_ntt(_p(a), len(a), int(inverse), device), "dilithium_ntt")
    return a


LANE_OPS = dict(KYBER_COMPRESS=1, KYBER_DECOMPRESS=2, KYBER_MSG_BIT=3, KYBER_MULC=4, KYBER_REDUCE32=5, KYBER_NORMALIZE=6, KYBER_CBD2_WORD=7,
                KYBER_DOT2=8, DIL_DECOMPOSE=9, DIL_USE_HINT=10, DIL_MAKE_HINT=11, DIL_POWER2ROUND=12, DIL_MONT32=13, DIL_MONT64=14,
                DIL_NORMALIZE=15, DIL_EXCEEDS=16)


def lane_op(op, a, b=None, arg=0, two=False, device=0):
    """The DEVICE instantiation of a coefficient-level function, elementwise over uint32 arrays -> out0 (, out1 with two=True)"""
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
    n = len(a)
    bb = None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.uint32), a.shape))
    o0 = np.empty(n, np.uint32)
    o1 = np.empty(n, np.uint32) if two else None
    nat.check(nat.lib().circl_hip_lane_op(LANE_OPS[op], int(arg), _p(a), None if bb is None else _p(bb), _p(o0), None if o1 is None else _p(o1), n, device),
              "lane_op " + op)
    return (o0, o1) if two else o0


def kyber_sample_uniform(seeds, xy, device=0):
    """Poly.DeriveUniform(seed_i, x_i, y_i) -> (n, 256) int16 in [0, q)"""
    seeds, xy = _u8(seeds, 32), _u8(xy, 2)
    out = np.empty((len(seeds), 256), np.int16)
    nat.check(nat.lib().circl_hip_kyber_sample_uniform(_p(seeds), _p(xy), _p(out), len(seeds), device), "kyber_sample_uniform")
    return out


def kyber_sample_cbd(eta, seeds, device=0):
    """Poly.DeriveNoise(seed_i, nonce, eta) for nonce 0..63 -> (n, 64, 256) int16 in [-eta, eta]"""
    seeds = _u8(seeds, 32)
    out = np.empty((len(seeds), 64, 256), np.int16)
    nat.check(nat.lib().circl_hip_kyber_sample_cbd(eta, _p(seeds), _p(out), len(seeds), device), "kyber_sample_cbd")
    return out


def mldsa_sample_uniform(seeds, nonces, device=0):
    """PolyDeriveUniform(seed_i, nonce_i) -> (n, 256) uint32 in [0, q)"""
    seeds = _u8(seeds, 32)
    nonces = np.ascontiguousarray(nonces, dtype=np.uint16).reshape(-1)
    assert len(nonces) == len(seeds)
    out = np.empty((len(seeds), 256), np.uint32)
    nat.check(nat.lib().circl_hip_mldsa_sample_uniform(_p(seeds), _p(nonces), _p(out), len(seeds), device), "mldsa_sample_uniform")
    return out


def shake(rate, ds, msgs, outlen, device=0):
    """msgs: (n, inlen) uint8 (equal lengths) -> (n, outlen)"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, inlen = msgs.shape
    out = np.empty((n, outlen), np.uint8)
    nat.check(nat.lib().circl_hip_shake(rate, ds, _p(msgs), inlen, _p(out), outlen, n, device), "shake")
    return out


def xof(rate, ds, msgs, outlen, rounds=24, device=0):
    """variable-length messages -> (n, outlen); rounds=12 gives TurboSHAKE"""
    n = len(msgs)
    mb, mo = _blob(msgs)
    out = np.empty((n, outlen), np.uint8)
    nat.check(nat.lib().circl_hip_xof(rate, ds, rounds, _p(mb), _p(mo), _p(out), outlen, n, device), "xof")
    return out


def k12(msgs, outlen, ctxs=None, device=0):
    """KangarooTwelve draft -10 of every message (xof/k12 Draft10Sum) -> (n, outlen)"""
    n = len(msgs)
    mb, mo = _blob(msgs)
    out = np.empty((n, outlen), np.uint8)
    if ctxs is None:
        rc = nat.lib().circl_hip_k12(_p(mb), _p(mo), None, None, _p(out), outlen, n, device)
    else:
        cb, co = _blob(ctxs)
        rc = nat.lib().circl_hip_k12(_p(mb), _p(mo), _p(cb), _p(co), _p(out), outlen, n, device)
    nat.check(rc, "k12")
    return out


def x25519(scalar, point=None, device=0):
    """Batch X25519 (dh/x25519): Shared(scalar_i, point_i), or KeyGen(scalar_i) when point is None.
    Returns (out (n, 32), ok (n,)): ok = 0 where the reference's Shared reports a low-order public key."""
    scalar = _u8(scalar, 32)
    n = scalar.shape[0]
    out = np.empty((n, 32), np.uint8)
    ok = np.empty(n, np.uint8)
    pt = None if point is None else _u8(point, 32)
    nat.check(nat.lib().circl_hip_x25519(_p(scalar), None if pt is None else _p(pt), _p(out), _p(ok), n, device), "x25519")
    return out, ok


XWING, X25519MLKEM768, KYBER768_X25519, KYBER512_X25519 = 1, 2, 3, 4
KYBER768_X448, KYBER1024_X448 = 5, 6  # hybrid.Kyber768X448() / Kyber1024X448(): X448 (56-byte rows) first, round-3 Kyber second
HYBRID_SIZES = {XWING: dict(seed=32, eseed=64, pk=1216, sk=32, ct=1120, ss=32), X25519MLKEM768: dict(seed=64, eseed=32, pk=1216, sk=2432, ct=1120, ss=64),
                KYBER768_X25519: dict(seed=64, eseed=32, pk=1216, sk=2432, ct=1120, ss=64),
                KYBER512_X25519: dict(seed=64, eseed=32, pk=832, sk=1664, ct=800, ss=64),
                KYBER768_X448: dict(seed=64, eseed=56, pk=1240, sk=2456, ct=1144, ss=88),
                KYBER1024_X448: dict(seed=64, eseed=56, pk=1624, sk=3224, ct=1624, ss=88)}


def hybrid_keygen(scheme, seeds, device=0):
    """X-Wing DeriveKeyPairPacked / kem/hybrid DeriveKeyPair (X25519MLKEM768, Kyber*-X25519, Kyber*-X448) for every seed -> (pk, sk)"""
    S = HYBRID_SIZES[scheme]
    seeds = _u8(seeds, S["seed"])
    n = seeds.shape[0]
    pk, sk = np.empty((n, S["pk"]), np.uint8), np.empty((n, S["sk"]), np.uint8)
    nat.check(nat.lib().circl_hip_hybrid_keygen(scheme, _p(seeds), _p(pk), _p(sk), n, device), "hybrid keygen")
    return pk, sk


def hybrid_encaps(scheme, pk, eseeds, device=0):
    """deterministic encapsulation -> (ct, ss, status)"""
    S = HYBRID_SIZES[scheme]
    pk, eseeds = _u8(pk, S["pk"]), _u8(eseeds, S["eseed"])
    n = pk.shape[0]
    ct, ss, st = np.empty((n, S["ct"]), np.uint8), np.empty((n, S["ss"]), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hybrid_encaps(scheme, _p(pk), _p(eseeds), _p(ct), _p(ss), _p(st), n, device), "hybrid encaps")
    return ct, ss, st


def hybrid_decaps(scheme, sk, ct, device=0):
    """-> (ss, status)"""
    S = HYBRID_SIZES[scheme]
    sk, ct = _u8(sk, S["sk"]), _u8(ct, S["ct"])
    n = sk.shape[0]
    ss, st = np.empty((n, S["ss"]), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hybrid_decaps(scheme, _p(sk), _p(ct), _p(ss), _p(st), n, device), "hybrid decaps")
    return ss, st


class CallQueue:
    """circl_hip_queue: the asynchronous form of the entry points that take their keys WITH the call (a TLS 1.3 server encapsulates to the client's
    ephemeral key).  op: "mlkem-encaps", "mlkem-decaps" (param 512 / 768 / 1024), "hybrid-encaps", "hybrid-decaps" (param = the hybrid scheme id)."""
    OPS = {"mlkem-encaps": 1, "mlkem-decaps": 2, "hybrid-encaps": 3, "hybrid-decaps": 4}

    def __init__(self, op, param, max_items, device=0, eventfd=False):
        import ctypes as C
        self.op, self.param = op, param
        self.handle = C.c_void_p()
        nat.check(nat.lib().circl_hip_queue_open(self.OPS[op], param, device, max_items, 1 if eventfd else 0, C.byref(self.handle)), "queue_open")

    def submit(self, key, inp, out0, ss, st):
        """(rc, ticket); key / inp: C-contiguous uint8 rows (copied before the call returns), out0 (None for a decapsulation) / ss / st: filled when the ticket is done"""
        import ctypes as C
        key, inp = np.ascontiguousarray(key, np.uint8), np.ascontiguousarray(inp, np.uint8)
        n = len(inp)
        t = C.c_uint64()
        rc = nat.lib().circl_hip_queue_submit(self.handle, _p(key), _p(inp), None if out0 is None else _p(out0), _p(ss), None if st is None else _p(st), n, C.byref(t))
        return rc, t.value

    def poll(self, tickets):
        t = np.asarray(tickets, np.uint64)
        st = np.zeros(len(t), np.int8)
        nat.lib().circl_hip_queue_poll(self.handle, _p(t), len(t), _p(st))
        return [int(x) for x in st]

    def wait(self, ticket, timeout_us=-1):
        return nat.lib().circl_hip_queue_wait(self.handle, int(ticket), int(timeout_us))

    def eventfd(self):
        return nat.lib().circl_hip_queue_eventfd(self.handle)

    def stats(self):
        import ctypes as C
        c, i, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        nat.check(nat.lib().circl_hip_queue_stats(self.handle, C.byref(c), C.byref(i), C.byref(l)), "queue_stats")
        return c.value, i.value, l.value

    def close(self):
        """CIRCL_HIP_OK (the queue is gone) or CIRCL_HIP_EBUSY"""
        rc = nat.lib().circl_hip_queue_close(self.handle)
        if rc == 0:
            self.handle = None
        return rc



def ed25519_keygen(seeds, device=0):
    """NewKeyFromSeed for every 32-byte seed -> (pk (n, 32), sk (n, 64) = seed || pk)"""
    seeds = _u8(seeds, 32)
    n = seeds.shape[0]
    pk, sk = np.empty((n, 32), np.uint8), np.empty((n, 64), np.uint8)
    nat.check(nat.lib().circl_hip_ed25519_keygen(_p(seeds), _p(pk), _p(sk), n, device), "ed25519_keygen")
    return pk, sk


def ed25519_sign(sk, msgs, device=0):
    """Sign(sk_i, msg_i) -> (n, 64)"""
    sk = _u8(sk, 64)
    n = sk.shape[0]
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    sig = np.empty((n, 64), np.uint8)
    nat.check(nat.lib().circl_hip_ed25519_sign(_p(sk), _p(mb), _p(mo), _p(sig), n, device), "ed25519_sign")
    return sig


def _rows_of_length(items, want):
    """(indices of the items of exactly `want` bytes, those items as an (m, want) array)"""
    items = [bytes(x) for x in items]
    idx = [i for i, x in enumerate(items) if len(x) == want]
    return idx, items


def _verify_fixed(fn, pk, sig, msgs, PK, SIG, where, device):
    """ok (n,): an item whose key is not PK bytes or whose signature is not SIG bytes is false without reaching the device, as in
    the reference; every other item is decided on the device"""
    n = len(msgs)
    pk_i, pk_l = _rows_of_length(pk, PK)
    sig_i, sig_l = _rows_of_length(sig, SIG)
    assert len(pk_l) == n and len(sig_l) == n
    idx = sorted(set(pk_i) & set(sig_i))
    ok = np.zeros(n, np.uint8)
    if idx:
        pka = np.frombuffer(b"".join(pk_l[i] for i in idx), np.uint8).reshape(-1, PK).copy()
        sga = np.frombuffer(b"".join(sig_l[i] for i in idx), np.uint8).reshape(-1, SIG).copy()
        mb, mo = _blob([msgs[i] for i in idx])
        sub = np.empty(len(idx), np.uint8)
        nat.check(fn(_p(pka), _p(sga), _p(mb), _p(mo), _p(sub), len(idx), device), where)
        ok[idx] = sub
    return ok


def ed25519_verify(pk, sig, msgs, device=0):
    """Verify(pk_i, msg_i, sig_i) -> ok (n,) of 0 / 1; pk and sig are sequences of byte strings or (n, 32) / (n, 64) arrays.
    Same argument order as mldsa_verify and the C ABI.  Wrong-length keys or signatures are false without a launch."""
    return _verify_fixed(nat.lib().circl_hip_ed25519_verify, pk, sig, msgs, 32, 64, "ed25519_verify", device)


def sha512(msgs, device=0):
    """SHA-512 of every message -> (n, 64)"""
    n = len(msgs)
    mb, mo = _blob(msgs)
    out = np.empty((n, 64), np.uint8)
    nat.check(nat.lib().circl_hip_sha512(_p(mb), _p(mo), _p(out), n, device), "sha512")
    return out


EDDILITHIUM2_SIZES = dict(pk=1344, sk=2560, sig=2484)


def eddilithium2_keygen(seeds, device=0):
    """sign/eddilithium2 NewKeyFromSeed for every 32-byte seed -> (pk (n, 1344), sk (n, 2560))"""
    seeds = _u8(seeds, 32)
    n = seeds.shape[0]
    pk, sk = np.empty((n, 1344), np.uint8), np.empty((n, 2560), np.uint8)
    nat.check(nat.lib().circl_hip_eddilithium2_keygen(_p(seeds), _p(pk), _p(sk), n, device), "eddilithium2_keygen")
    return pk, sk


def eddilithium2_sign(sk, msgs, device=0):
    """SignTo(sk_i, msg_i) -> (n, 2484) = deterministic Dilithium2 signature || Ed25519 signature"""
    sk = _u8(sk, 2560)
    n = sk.shape[0]
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    sig = np.empty((n, 2484), np.uint8)
    nat.check(nat.lib().circl_hip_eddilithium2_sign(_p(sk), _p(mb), _p(mo), _p(sig), n, device), "eddilithium2_sign")
    return sig


def eddilithium2_verify(pk, sig, msgs, device=0):
    """Verify(pk_i, msg_i, sig_i) -> ok (n,): both halves must verify; wrong lengths are false without a launch"""
    return _verify_fixed(nat.lib().circl_hip_eddilithium2_verify, pk, sig, msgs, 1344, 2484, "eddilithium2_verify", device)


def x448(scalar, point=None, device=0):
    """Batch X448 (dh/x448): Shared(scalar_i, point_i), or KeyGen(scalar_i) when point is None.
    Returns (out (n, 56), ok (n,)): ok = 0 where the reference's Shared reports a low-order public key."""
    scalar = _u8(scalar, 56)
    n = scalar.shape[0]
    out = np.empty((n, 56), np.uint8)
    ok = np.empty(n, np.uint8)
    pt = None if point is None else _u8(point, 56)
    nat.check(nat.lib().circl_hip_x448(_p(scalar), None if pt is None else _p(pt), _p(out), _p(ok), n, device), "x448")
    return out, ok


def ed448_keygen(seeds, device=0):
    """sign/ed448 NewKeyFromSeed for every 57-byte seed -> (pk (n, 57), sk (n, 114) = seed || pk)"""
    seeds = _u8(seeds, 57)
    n = seeds.shape[0]
    pk, sk = np.empty((n, 57), np.uint8), np.empty((n, 114), np.uint8)
    nat.check(nat.lib().circl_hip_ed448_keygen(_p(seeds), _p(pk), _p(sk), n, device), "ed448_keygen")
    return pk, sk


def _ctx_args(ctxs, n):
    """(blob pointer, offsets pointer, keep-alive) for a list of n contexts, or NULLs for None (every context empty)"""
    if ctxs is None:
        return None, None, None
    assert len(ctxs) == n
    cb, co = _blob(ctxs)
    return _p(cb), _p(co), (cb, co)


def ed448_sign(sk, msgs, ctxs=None, device=0):
    """Sign(sk_i, msg_i, ctx_i) -> (n, 114); ctxs=None: every context empty.  A context over 255 bytes raises (the reference
    panics)."""
    sk = _u8(sk, 114)
    n = sk.shape[0]
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    cb, co, _keep = _ctx_args(ctxs, n)
    sig = np.empty((n, 114), np.uint8)
    nat.check(nat.lib().circl_hip_ed448_sign(_p(sk), _p(mb), _p(mo), cb, co, _p(sig), n, device), "ed448_sign")
    return sig


def ed448_verify(pk, sig, msgs, ctxs=None, device=0):
    """Verify(pk_i, msg_i, sig_i, ctx_i) -> ok (n,) of 0 / 1; pk and sig are sequences of byte strings or (n, 57) / (n, 114)
    arrays; ctxs=None: every context empty.  Wrong-length keys or signatures are false without a launch; a context over 255 bytes
    is false."""
    n = len(msgs)
    pk_i, pk_l = _rows_of_length(pk, 57)
    sig_i, sig_l = _rows_of_length(sig, 114)
    assert len(pk_l) == n and len(sig_l) == n and (ctxs is None or len(ctxs) == n)
    idx = sorted(set(pk_i) & set(sig_i))
    ok = np.zeros(n, np.uint8)
    if idx:
        pka = np.frombuffer(b"".join(pk_l[i] for i in idx), np.uint8).reshape(-1, 57).copy()
        sga = np.frombuffer(b"".join(sig_l[i] for i in idx), np.uint8).reshape(-1, 114).copy()
        mb, mo = _blob([msgs[i] for i in idx])
        cb, co, _keep = _ctx_args(None if ctxs is None else [ctxs[i] for i in idx], len(idx))
        sub = np.empty(len(idx), np.uint8)
        nat.check(nat.lib().circl_hip_ed448_verify(_p(pka), _p(sga), _p(mb), _p(mo), cb, co, _p(sub), len(idx), device), "ed448_verify")
        ok[idx] = sub
    return ok


EDDILITHIUM3_SIZES = dict(seed=57, pk=2009, sk=4057, sig=3407)


def eddilithium3_keygen(seeds, device=0):
    """sign/eddilithium3 NewKeyFromSeed for every 57-byte seed -> (pk (n, 2009), sk (n, 4057))"""
    seeds = _u8(seeds, 57)
    n = seeds.shape[0]
    pk, sk = np.empty((n, 2009), np.uint8), np.empty((n, 4057), np.uint8)
    nat.check(nat.lib().circl_hip_eddilithium3_keygen(_p(seeds), _p(pk), _p(sk), n, device), "eddilithium3_keygen")
    return pk, sk


def eddilithium3_sign(sk, msgs, device=0):
    """SignTo(sk_i, msg_i) -> (n, 3407) = deterministic Dilithium3 signature || Ed448 signature (empty context)"""
    sk = _u8(sk, 4057)
    n = sk.shape[0]
    assert len(msgs) == n
    mb, mo = _blob(msgs)
    sig = np.empty((n, 3407), np.uint8)
    nat.check(nat.lib().circl_hip_eddilithium3_sign(_p(sk), _p(mb), _p(mo), _p(sig), n, device), "eddilithium3_sign")
    return sig


def eddilithium3_verify(pk, sig, msgs, device=0):
    """Verify(pk_i, msg_i, sig_i) -> ok (n,): both halves must verify; wrong lengths are false without a launch"""
    return _verify_fixed(nat.lib().circl_hip_eddilithium3_verify, pk, sig, msgs, 2009, 3407, "eddilithium3_verify", device)


FRODO640SHAKE_SIZES = dict(pk=9616, sk=19888, ct=9720, ss=16, seed=48, eseed=16)


def _frodo_rows(x, cols, what):
    """an (n, cols) uint8 array from a 2-D array or a sequence of byte strings; any row of another length is refused here, before
    anything is launched (the reference panics or returns kem.ErrCiphertextSize / ErrSeedSize, frodo.go:517-547)"""
    if isinstance(x, np.ndarray):
        if x.ndim != 2 or x.shape[1] != cols:
            raise ValueError("frodo640shake: %s must be rows of %d bytes, got shape %r" % (what, cols, x.shape))
        return np.ascontiguousarray(x, dtype=np.uint8)
    items = [x] if isinstance(x, (bytes, bytearray, memoryview)) else list(x)
    for it in items:
        if len(it) != cols:
            raise ValueError("frodo640shake: %s must be %d bytes, got %d" % (what, cols, len(it)))
    return np.frombuffer(b"".join(bytes(it) for it in items), np.uint8).reshape(len(items), cols).copy()


def frodo640shake_keygen(seeds, device=0):
    """kem/frodo/frodo640shake DeriveKeyPair for every 48-byte seed (s || seedSE || z) -> (pk (n, 9616), sk (n, 19888))"""
    seeds = _frodo_rows(seeds, 48, "a key seed")
    n = seeds.shape[0]
    pk, sk = np.empty((n, 9616), np.uint8), np.empty((n, 19888), np.uint8)
    nat.check(nat.lib().circl_hip_frodo640shake_keygen(_p(seeds), _p(pk), _p(sk), n, device), "frodo640shake_keygen")
    return pk, sk


def frodo640shake_encaps(pk, seeds, device=0):
    """EncapsulateDeterministically(pk_i, seed_i) (16-byte seeds) -> (ct (n, 9720), ss (n, 16))"""
    pk = _frodo_rows(pk, 9616, "a public key")
    seeds = _frodo_rows(seeds, 16, "an encapsulation seed")
    n = pk.shape[0]
    if seeds.shape[0] != n:
        raise ValueError("frodo640shake: %d public keys, %d seeds" % (n, seeds.shape[0]))
    ct, ss = np.empty((n, 9720), np.uint8), np.empty((n, 16), np.uint8)
    nat.check(nat.lib().circl_hip_frodo640shake_encaps(_p(pk), _p(seeds), _p(ct), _p(ss), n, device), "frodo640shake_encaps")
    return ct, ss


def frodo640shake_decaps(sk, ct, device=0):
    """Decapsulate(sk_i, ct_i) -> ss (n, 16); a ciphertext that does not re-encrypt gives SHAKE128(ct || s), as in the reference"""
    sk = _frodo_rows(sk, 19888, "a private key")
    ct = _frodo_rows(ct, 9720, "a ciphertext")
    n = sk.shape[0]
    if ct.shape[0] != n:
        raise ValueError("frodo640shake: %d private keys, %d ciphertexts" % (n, ct.shape[0]))
    ss = np.empty((n, 16), np.uint8)
    nat.check(nat.lib().circl_hip_frodo640shake_decaps(_p(sk), _p(ct), _p(ss), n, device), "frodo640shake_decaps")
    return ss


def sha256(msgs, device=0):
    """SHA-256 of every message -> (n, 32)"""
    n = len(msgs)
    mb, mo = _blob(msgs)
    out = np.empty((n, 32), np.uint8)
    nat.check(nat.lib().circl_hip_sha256(_p(mb), _p(mo), _p(out), n, device), "sha256")
    return out


# ---- HPKE DHKEM over X25519 / HKDF-SHA256 (0x20) and X448 / HKDF-SHA512 (0x21): hpke/kembase.go, hpke/xkem.go ----
HPKE_KEM_X25519_HKDF_SHA256, HPKE_KEM_X448_HKDF_SHA512 = 0x20, 0x21
HPKE_DHKEM_SIZES = {0x20: dict(key=32, ss=32), 0x21: dict(key=56, ss=64)}


def _hpke_rows(kem, *rows):
    if kem not in HPKE_DHKEM_SIZES:
        raise ValueError("unknown HPKE KEM id 0x%x (0x20 = X25519/HKDF-SHA256, 0x21 = X448/HKDF-SHA512)" % kem)
    N = HPKE_DHKEM_SIZES[kem]["key"]
    out = [None if r is None else _u8(r, N) for r in rows]
    n = out[0].shape[0]
    if any(r is not None and r.shape[0] != n for r in out):
        raise ValueError("hpke_dhkem: the inputs differ in their number of rows")
    return N, HPKE_DHKEM_SIZES[kem]["ss"], n, out


def _po(a):
    return None if a is None else _p(a)


def hpke_dhkem_derive_keypair(kem, ikm, device=0):
    """xKEM.DeriveKeyPair(ikm_i) -> (sk (n, N), pk (n, N)); sk is the raw LabeledExpand output (unclamped), as the reference stores it.
    GenerateKeyPair is x25519() / x448() with point=None on sk rows drawn by the caller."""
    N, _, n, (ikm,) = _hpke_rows(kem, ikm)
    sk, pk = np.empty((n, N), np.uint8), np.empty((n, N), np.uint8)
    nat.check(nat.lib().circl_hip_hpke_dhkem_derive_keypair(kem, _p(ikm), _p(sk), _p(pk), n, device), "hpke_dhkem_derive_keypair")
    return sk, pk


def hpke_dhkem_encap(kem, pkR, ikmE, device=0):
    """EncapsulateDeterministically(pkR_i, ikmE_i) -> (enc (n, N), ss (n, S), ok (n,)); ok = 0 (and zero rows) for a low-order pkR"""
    N, S, n, (pkR, ikmE) = _hpke_rows(kem, pkR, ikmE)
    enc, ss, ok = np.empty((n, N), np.uint8), np.empty((n, S), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hpke_dhkem_encap(kem, _p(pkR), _p(ikmE), _p(enc), _p(ss), _p(ok), n, device), "hpke_dhkem_encap")
    return enc, ss, ok


def hpke_dhkem_decap(kem, skR, enc, pkR=None, device=0):
    """Decapsulate(skR_i, enc_i) -> (ss (n, S), ok (n,)); pkR = skR's public key if the caller has it (else it is computed)"""
    N, S, n, (skR, enc, pkR) = _hpke_rows(kem, skR, enc, pkR)
    ss, ok = np.empty((n, S), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hpke_dhkem_decap(kem, _p(skR), _po(pkR), _p(enc), _p(ss), _p(ok), n, device), "hpke_dhkem_decap")
    return ss, ok


def hpke_dhkem_auth_encap(kem, pkR, skS, ikmE, pkS=None, device=0):
    """AuthEncapsulateDeterministically(pkR_i, skS_i, ikmE_i) -> (enc, ss, ok); pkS = skS's public key if the caller has it"""
    N, S, n, (pkR, skS, ikmE, pkS) = _hpke_rows(kem, pkR, skS, ikmE, pkS)
    enc, ss, ok = np.empty((n, N), np.uint8), np.empty((n, S), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hpke_dhkem_auth_encap(kem, _p(pkR), _p(skS), _po(pkS), _p(ikmE), _p(enc), _p(ss), _p(ok), n, device),
              "hpke_dhkem_auth_encap")
    return enc, ss, ok


def hpke_dhkem_auth_decap(kem, skR, enc, pkS, pkR=None, device=0):
    """AuthDecapsulate(skR_i, enc_i, pkS_i) -> (ss, ok); pkR = skR's public key if the caller has it"""
    N, S, n, (skR, enc, pkS, pkR) = _hpke_rows(kem, skR, enc, pkS, pkR)
    ss, ok = np.empty((n, S), np.uint8), np.empty(n, np.uint8)
    nat.check(nat.lib().circl_hip_hpke_dhkem_auth_decap(kem, _p(skR), _po(pkR), _p(enc), _p(pkS), _p(ss), _p(ok), n, device), "hpke_dhkem_auth_decap")
    return ss, ok


# ---- HPKE contexts: key schedule, ChaCha20-Poly1305 Seal / Open, Export (hpke/hpke.go, hpke/util.go, hpke/aead.go) ----
HPKE_KDF_HKDF_SHA256, HPKE_KDF_HKDF_SHA512 = 1, 3
HPKE_AEAD_CHACHA20POLY1305, HPKE_AEAD_EXPORT_ONLY = 3, 0xFFFF
HPKE_MODE_BASE, HPKE_MODE_PSK, HPKE_MODE_AUTH, HPKE_MODE_AUTH_PSK = range(4)


def hpke_context_size(kdf):
    return nat.lib().circl_hip_hpke_context_size(kdf)


def _rag(items, n):
    """a list of byte strings (or None: every item empty) -> (blob, offsets) arrays or (None, None)"""
    if items is None:
        return None, None
    if len(items) != n:
        raise ValueError("hpke: a ragged input has %d items, the call %d" % (len(items), n))
    return _blob(items)


def _unrag(blob, off, extra=0):
    return [blob[int(off[k]) + extra * k:int(off[k + 1]) + extra * (k + 1)].tobytes() for k in range(len(off) - 1)]


class HpkeSuite:
    """One HPKE suite (kem, kdf, aead) on host buffers.  Key rows are (n, N) arrays or byte strings; info, psk, psk_id, aad, plaintexts and
    exporter contexts are lists of n byte strings (None: every item empty).  Failed items (a low-order point, the psk rule, a tag that does
    not verify) have ok = 0 and zero outputs.  The caller owns the sequence numbers of a context."""

    def __init__(self, kem, kdf, aead, device=0):
        self.kem, self.kdf, self.aead, self.device = kem, kdf, aead, device
        self.CS = hpke_context_size(kdf)
        if kem not in HPKE_DHKEM_SIZES or not self.CS or aead not in (HPKE_AEAD_CHACHA20POLY1305, HPKE_AEAD_EXPORT_ONLY):
            raise ValueError("HPKE suite (0x%x, 0x%x, 0x%x) is not served" % (kem, kdf, aead))
        self.N = HPKE_DHKEM_SIZES[kem]["key"]
        self.L = nat.lib()

    def _setup_args(self, mode, rows, info, psk, psk_id):
        _, _, n, rows = _hpke_rows(self.kem, *rows)
        rag = [_rag(x, n) for x in (info, psk, psk_id)]
        keep = (rows, rag)
        args = [self.kem, self.kdf, self.aead, mode] + [_po(r) for r in rows] + [_po(a) for pair in rag for a in pair]
        return n, args, keep

    def setup_sender(self, mode, pkR, ikmE, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        """-> (enc (n, N), ctx (n, context size), ok (n,))"""
        n, args, keep = self._setup_args(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id)
        enc, ctx, ok = np.empty((n, self.N), np.uint8), np.empty((n, self.CS), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_setup_sender(*args, _p(enc), _p(ctx), _p(ok), n, self.device), "hpke_setup_sender")
        return enc, ctx, ok

    def setup_receiver(self, mode, skR, enc, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        """-> (ctx, ok)"""
        n, args, keep = self._setup_args(mode, (skR, pkR, enc, pkS), info, psk, psk_id)
        ctx, ok = np.empty((n, self.CS), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_setup_receiver(*args, _p(ctx), _p(ok), n, self.device), "hpke_setup_receiver")
        return ctx, ok

    @staticmethod
    def _seq(seq, n):
        return None if seq is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seq, np.uint64), (n,)))

    def seal(self, ctx, pts, aads=None, seq=None):
        """-> the n ciphertexts (ct || tag) as byte strings"""
        ctx = _u8(ctx, self.CS)
        n = ctx.shape[0]
        (pb, po), (ab, ao), sq = _rag(pts, n), _rag(aads, n), self._seq(seq, n)
        ct = np.empty(int(po[n]) + 16 * n, np.uint8)
        nat.check(self.L.circl_hip_hpke_seal(self.aead, _p(ctx), self.CS, _po(sq), _p(pb), _p(po), _po(ab), _po(ao), _p(ct), n, self.device), "hpke_seal")
        return _unrag(ct, po, 16)

    def open(self, ctx, cts, aads=None, seq=None):
        """-> (the n plaintexts as byte strings, ok (n,)); a ciphertext shorter than a tag is refused here"""
        ctx = _u8(ctx, self.CS)
        n = ctx.shape[0]
        if len(cts) != n or any(len(c) < 16 for c in cts):
            raise ValueError("hpke_open: need %d ciphertexts of at least 16 bytes" % n)
        cb, _ = _blob(cts)
        _, po = _blob([bytes(len(c) - 16) for c in cts])
        (ab, ao), sq = _rag(aads, n), self._seq(seq, n)
        pt, ok = np.empty(int(po[n]) + 1, np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_open(self.aead, _p(ctx), self.CS, _po(sq), _p(cb), _p(po), _po(ab), _po(ao), _p(pt), _p(ok), n, self.device), "hpke_open")
        return _unrag(pt, po), ok

    def export(self, ctx, exporter_contexts, length):
        """-> (n, length)"""
        ctx = _u8(ctx, self.CS)
        n = ctx.shape[0]
        eb, eo = _rag(exporter_contexts, n)
        out = np.empty((n, max(length, 0)), np.uint8)
        nat.check(self.L.circl_hip_hpke_export(self.kdf, self.kem, self.aead, _p(ctx), self.CS, _po(eb), _po(eo), length, _p(out), n, self.device), "hpke_export")
        return out

    def seal_single(self, mode, pkR, ikmE, pts, aads=None, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        """RFC 9180 section 6 Seal<MODE> -> (enc, the n ciphertexts, ok)"""
        n, args, keep = self._setup_args(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id)
        (pb, po), (ab, ao) = _rag(pts, n), _rag(aads, n)
        enc, ct, ok = np.empty((n, self.N), np.uint8), np.empty(int(po[n]) + 16 * n, np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_seal_single(*args, _p(pb), _p(po), _po(ab), _po(ao), _p(enc), _p(ct), _p(ok), n, self.device), "hpke_seal_single")
        return enc, _unrag(ct, po, 16), ok

    def open_single(self, mode, skR, enc, cts, aads=None, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        """RFC 9180 section 6 Open<MODE> -> (the n plaintexts, ok)"""
        n, args, keep = self._setup_args(mode, (skR, pkR, enc, pkS), info, psk, psk_id)
        if len(cts) != n or any(len(c) < 16 for c in cts):
            raise ValueError("hpke_open_single: need %d ciphertexts of at least 16 bytes" % n)
        cb, _ = _blob(cts)
        _, po = _blob([bytes(len(c) - 16) for c in cts])
        ab, ao = _rag(aads, n)
        pt, ok = np.empty(int(po[n]) + 1, np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_open_single(*args, _p(cb), _p(po), _po(ab), _po(ao), _p(pt), _p(ok), n, self.device), "hpke_open_single")
        return _unrag(pt, po), ok

    def export_single(self, mode, pkR, ikmE, exporter_contexts, length, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        """RFC 9180 section 6 SendExport<MODE> -> (enc, exported (n, length), ok)"""
        n, args, keep = self._setup_args(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id)
        eb, eo = _rag(exporter_contexts, n)
        enc, out, ok = np.empty((n, self.N), np.uint8), np.empty((n, max(length, 0)), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_export_single(*args, _po(eb), _po(eo), length, _p(enc), _p(out), _p(ok), n, self.device), "hpke_export_single")
        return enc, out, ok

    def export_single_receiver(self, mode, skR, enc, exporter_contexts, length, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        """RFC 9180 section 6 ReceiveExport<MODE> -> (exported (n, length), ok)"""
        n, args, keep = self._setup_args(mode, (skR, pkR, enc, pkS), info, psk, psk_id)
        eb, eo = _rag(exporter_contexts, n)
        out, ok = np.empty((n, max(length, 0)), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_hpke_export_single_receiver(*args, _po(eb), _po(eo), length, _p(out), _p(ok), n, self.device), "hpke_export_single_receiver")
        return out, ok


# ---- ristretto255 (group/ristretto255.go), NIST P-256 / P-384 (group/short.go) and base-mode OPRF on them (oprf/keys.go, client.go, server.go;
# RFC 9497, suites ristretto255-SHA512, P256-SHA256 and P384-SHA384) ----
OPRF_MODE_OPRF, OPRF_MODE_VOPRF, OPRF_MODE_POPRF = range(3)
R255_INVERT = 1


def _scalar_rows(x, n=None, width=32):
    """(rows, stride): one scalar of `width` bytes (bytes or a (width,) / (1, width) array with n given) is shared by the batch, stride 0"""
    a = _u8(x, width)
    if n is not None and len(a) == 1 and n != 1:
        return a, 0
    if n is not None and len(a) != n:
        raise ValueError("need 1 or %d scalar rows, got %d" % (n, len(a)))
    return a, width


class _OprfSuite:
    """The group operations and the proof-free part of OPRF for one suite of the C ABI, written once.  The ristretto255_* / oprf_*
    functions below and NistpOprf bind it.  group / oprf: the prefixes of the symbols (and of the names in error messages); lead: the
    arguments every call starts with (the curve id, or none); Ns / Ne / Nh: bytes of a scalar, an element, an output; tail: the end of the
    context string; nonuniform: hash_to_group takes a flags argument; err: what a ValueError of finalize is named by."""

    def __init__(self, group, oprf, lead, Ns, Ne, Nh, tail, nonuniform, err):
        self.group, self.oprf, self.lead, self.Ns, self.Ne, self.Nh, self.tail, self.nonuniform, self.err = group, oprf, lead, Ns, Ne, Nh, tail, nonuniform, err

    def _call(self, name, *args):
        nat.check(getattr(nat.lib(), "circl_hip_" + name)(*self.lead, *args), name)

    def context_string(self, mode):
        return b"OPRFV1-" + bytes([mode]) + self.tail

    def _hash(self, name, width, msgs, dst, flags, device):
        n = len(msgs)
        (mb, mo), d, out = _blob(msgs), np.frombuffer(bytes(dst) + b"\0", np.uint8), np.empty((n, width), np.uint8)
        self._call(self.group + name, _p(mb), _p(mo), _p(d), len(dst), *flags, _p(out), n, device)
        return out

    def hash_to_group(self, msgs, dst, nonuniform, device):
        return self._hash("_hash_to_group", self.Ne, msgs, dst, (1 if nonuniform else 0,) if self.nonuniform else (), device)

    def hash_to_scalar(self, msgs, dst, device):
        return self._hash("_hash_to_scalar", self.Ns, msgs, dst, (), device)

    def scalar_mult(self, scalars, elems, invert, n, device):
        elems = None if elems is None else _u8(elems, self.Ne)
        n = len(elems) if elems is not None else n
        sc, stride = _scalar_rows(scalars, n, self.Ns)
        n = len(sc) if n is None else n
        out, ok = np.empty((n, self.Ne), np.uint8), np.empty(n, np.uint8)
        self._call(self.group + "_scalar_mult", _p(sc), stride, _po(elems), R255_INVERT if invert else 0, _p(out), _p(ok), n, device)
        return out, ok

    def derive_keypair(self, mode, seeds, infos, device):
        seeds = _u8(seeds, 32)
        n = len(seeds)
        (ib, io), sk, pk, ok = _rag(infos, n), np.empty((n, self.Ns), np.uint8), np.empty((n, self.Ne), np.uint8), np.empty(n, np.uint8)
        self._call(self.oprf + "_derive_keypair", mode, _p(seeds), _po(ib), _po(io), _p(sk), _p(pk), _p(ok), n, device)
        return sk, pk, ok

    def blind(self, mode, inputs, blinds, device):
        blinds = _u8(blinds, self.Ns)
        n = len(blinds)
        (ib, io), out, ok = _rag(inputs, n), np.empty((n, self.Ne), np.uint8), np.empty(n, np.uint8)
        self._call(self.oprf + "_blind", mode, _po(ib), _po(io), _p(blinds), _p(out), _p(ok), n, device)
        return out, ok

    def evaluate(self, sk, blinded, device):
        blinded = _u8(blinded, self.Ne)
        n = len(blinded)
        (key, stride), out, ok = _scalar_rows(sk, n, self.Ns), np.empty((n, self.Ne), np.uint8), np.empty(n, np.uint8)
        self._call(self.oprf + "_evaluate", _p(key), stride, _p(blinded), _p(out), _p(ok), n, device)
        return out, ok

    def finalize(self, inputs, blinds, evaluated, device):
        blinds, evaluated = _u8(blinds, self.Ns), _u8(evaluated, self.Ne)
        n = len(blinds)
        if len(evaluated) != n:
            raise ValueError("%sfinalize: %d blinds, %d evaluated elements" % (self.err, n, len(evaluated)))
        (ib, io), out, ok = _rag(inputs, n), np.empty((n, self.Nh), np.uint8), np.empty(n, np.uint8)
        self._call(self.oprf + "_finalize", _po(ib), _po(io), _p(blinds), _p(evaluated), _p(out), _p(ok), n, device)
        return out, ok

    def full_evaluate(self, mode, sk, inputs, device):
        n = len(inputs)
        (key, stride), (ib, io), out, ok = _scalar_rows(sk, n, self.Ns), _blob(inputs), np.empty((n, self.Nh), np.uint8), np.empty(n, np.uint8)
        self._call(self.oprf + "_full_evaluate", mode, _p(key), stride, _p(ib), _p(io), _p(out), _p(ok), n, device)
        return out, ok


_R255 = _OprfSuite("ristretto255", "oprf", (), 32, 32, 64, b"-ristretto255-SHA512", False, "oprf_")


def ristretto255_hash_to_group(msgs, dst, device=0):
    """Ristretto255.HashToElement(msg_i, dst) -> (n, 32); one dst of 1..255 bytes for the batch"""
    return _R255.hash_to_group(msgs, dst, False, device)


def ristretto255_hash_to_scalar(msgs, dst, device=0):
    """Ristretto255.HashToScalar(msg_i, dst) -> (n, 32)"""
    return _R255.hash_to_scalar(msgs, dst, device)


def ristretto255_scalar_mult(scalars, elems=None, invert=False, n=None, device=0):
    """scalar_i elem_i (elems None: the generator; invert: by scalar_i^-1) -> (out (n, 32), ok (n,)).  One scalar row with n (or with
    several elems) is shared by the batch.  ok = 0 and a zero row for an element that does not decode, a scalar >= L, an inverse of 0."""
    return _R255.scalar_mult(scalars, elems, invert, n, device)


def oprf_derive_keypair(mode, seeds, infos=None, device=0):
    """oprf.DeriveKey(suite, mode, seed_i, info_i) -> (sk (n, 32), pk (n, 32), ok (n,))"""
    return _R255.derive_keypair(mode, seeds, infos, device)


def oprf_blind(mode, inputs, blinds, device=0):
    """Client.DeterministicBlind: blind_i HashToGroup(input_i) -> (blinded (n, 32), ok (n,)); the caller draws the blinds"""
    return _R255.blind(mode, inputs, blinds, device)


def oprf_evaluate(sk, blinded, device=0):
    """base-mode Server.Evaluate: sk blinded_i -> (evaluated (n, 32), ok (n,)); sk = one key for the batch (32 bytes) or (n, 32) rows"""
    return _R255.evaluate(sk, blinded, device)


def oprf_finalize(inputs, blinds, evaluated, device=0):
    """base-mode Client.Finalize -> (outputs (n, 64), ok (n,))"""
    return _R255.finalize(inputs, blinds, evaluated, device)


def oprf_full_evaluate(mode, sk, inputs, device=0):
    """Server.FullEvaluate (mode 0) / VerifiableServer.FullEvaluate (mode 1) -> (outputs (n, 64), ok (n,)); sk as in oprf_evaluate"""
    return _R255.full_evaluate(mode, sk, inputs, device)


class NistpOprf:
    """The group operations and the proof-free part of OPRF on one NIST curve (circl_hip_nistp_*, circl_hip_oprf_nistp_*), shaped like the
    ristretto255 functions above.  curve = 256 or 384.  Scalars, keys and blinds are big-endian rows of Ns = 32 / 48 bytes, elements SEC 1
    compressed rows of Ne = 33 / 49 (the identity: the zero row), seeds rows of 32, OPRF outputs rows of Nh = 32 / 48.  A single scalar row
    is shared by the batch.  Failed items have ok = 0 and zero rows."""

    def __init__(self, curve, device=0):
        if curve not in (256, 384):
            raise ValueError("curve is 256 or 384")
        self.curve, self.device = curve, device
        self.Ns = curve // 8
        self.Ne, self.Nh = self.Ns + 1, self.Ns
        self._s = _OprfSuite("nistp", "oprf_nistp", (curve,), self.Ns, self.Ne, self.Nh, b"-P256-SHA256" if curve == 256 else b"-P384-SHA384", True, "")

    def context_string(self, mode):
        return self._s.context_string(mode)

    def hash_to_group(self, msgs, dst, nonuniform=False):
        """HashToElement(msg_i, dst) (nonuniform: HashToElementNonUniform) -> (n, Ne); one dst of 1..255 bytes for the batch"""
        return self._s.hash_to_group(msgs, dst, nonuniform, self.device)

    def hash_to_scalar(self, msgs, dst):
        """HashToScalar(msg_i, dst) -> (n, Ns)"""
        return self._s.hash_to_scalar(msgs, dst, self.device)

    def scalar_mult(self, scalars, elems=None, invert=False, n=None):
        """scalar_i elem_i (elems None: the generator; invert: by scalar_i^-1) -> (out (n, Ne), ok (n,))"""
        return self._s.scalar_mult(scalars, elems, invert, n, self.device)

    def derive_keypair(self, mode, seeds, infos=None):
        """oprf.DeriveKey(suite, mode, seed_i, info_i) -> (sk (n, Ns), pk (n, Ne), ok (n,))"""
        return self._s.derive_keypair(mode, seeds, infos, self.device)

    def blind(self, mode, inputs, blinds):
        """Client.DeterministicBlind -> (blinded (n, Ne), ok (n,)); the caller draws the blinds"""
        return self._s.blind(mode, inputs, blinds, self.device)

    def evaluate(self, sk, blinded):
        """base-mode Server.Evaluate -> (evaluated (n, Ne), ok (n,)); sk = one key for the batch or (n, Ns) rows"""
        return self._s.evaluate(sk, blinded, self.device)

    def finalize(self, inputs, blinds, evaluated):
        """base-mode Client.Finalize -> (outputs (n, Nh), ok (n,))"""
        return self._s.finalize(inputs, blinds, evaluated, self.device)

    def full_evaluate(self, mode, sk, inputs):
        """Server.FullEvaluate (mode 0) / VerifiableServer.FullEvaluate (mode 1) -> (outputs (n, Nh), ok (n,)); sk as in evaluate"""
        return self._s.full_evaluate(mode, sk, inputs, self.device)

    # the DLEQ proofs and the verifiable modes (circl_hip_nistp_dleq_*, circl_hip_oprf_nistp_poprf_*): proofs are rows of 2 Ns bytes, c || s
    def dleq_prove(self, k, kA, B, kB, req_off, r, dst, flags=0):
        """ProveBatchWithRandomnessRFC9497 per request -> (proofs (n_req, 2 Ns), ok (n_req,)); the arguments of dleq_prove"""
        return _DleqSuite(self._s).prove(k, kA, B, kB, req_off, r, dst, flags, self.device)

    def dleq_verify(self, kA, B, kB, req_off, proofs, dst, flags=0):
        """VerifyBatchRFC9497 per request -> ok (n_req,), the verdicts"""
        return _DleqSuite(self._s).verify(kA, B, kB, req_off, proofs, dst, flags, self.device)

    def poprf_tweak(self, infos, sk=None, pkS=None):
        """mode 2.  With sk -> (t, t_inv, t G, ok); with pkS -> (tweaked key, ok).  One key or n rows."""
        return _DleqSuite(self._s).poprf_tweak(infos, sk, pkS, self.device)

    def poprf_finalize(self, inputs, infos, blinds, evaluated):
        """PartialObliviousClient.Finalize without the proof -> (outputs (n, Nh), ok (n,))"""
        return _DleqSuite(self._s).poprf_finalize(inputs, infos, blinds, evaluated, self.device)

    def poprf_full_evaluate(self, sk, inputs, infos):
        """PartialObliviousServer.FullEvaluate -> (outputs (n, Nh), ok (n,)); sk as in evaluate"""
        return _DleqSuite(self._s).poprf_full_evaluate(sk, inputs, infos, self.device)

    def evaluate_verifiable(self, mode, sk, blinded, req_off, r, info=b""):
        """VerifiableServer.Evaluate (mode 1) / PartialObliviousServer.Evaluate (mode 2) under ONE key (and one info) ->
        (evaluated (n_elems, Ne), proofs (n_req, 2 Ns), ok (n_req,)); as oprf_evaluate_verifiable"""
        return _DleqSuite(self._s).evaluate_verifiable(mode, sk, blinded, req_off, r, info, self.device)

    def finalize_verifiable(self, mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info=b""):
        """VerifiableClient.Finalize (mode 1) / PartialObliviousClient.Finalize (mode 2) -> (outputs (n_elems, Nh), ok (n_req,)); the outputs
        of every element of a request whose proof or any element failed are zero"""
        return _DleqSuite(self._s).finalize_verifiable(mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info, self.device)


# ---- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms) and the verifiable modes of OPRF (VOPRF, POPRF) --------------------------------
DLEQ_NO_IDENTITY = 1


def oprf_context_string(mode):
    return _R255.context_string(mode)


def _req_off(req_off):
    off = np.ascontiguousarray(req_off, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("req_off: need n_req + 1 offsets")
    return off, len(off) - 1


def _elems(x, off, width=32):
    a = _u8(x, width) if len(x) else np.zeros((0, width), np.uint8)
    if len(a) != int(off[-1]):
        raise ValueError("%d element rows, the offsets end at %d" % (len(a), int(off[-1])))
    return a if len(a) else np.zeros((1, width), np.uint8)      # (an address even for a call of empty requests)


def _per_element(off, rows):
    """the per-request rows repeated for every element of their request"""
    return np.repeat(rows, np.diff(off.astype(np.int64)), axis=0)


class _DleqSuite:
    """The DLEQ proofs, the mode-2 (POPRF) items and the verifiable modes of OPRF for one suite of the C ABI, written once over an
    _OprfSuite.  The dleq_* / oprf_poprf_* / oprf_*_verifiable functions below and the methods of NistpOprf bind it."""

    def __init__(self, suite):
        self.s = suite
        self.dleq = "dleq" if suite.group == "ristretto255" else suite.group + "_dleq"       # the prefixes of the symbols

    def prove(self, k, kA, B, kB, req_off, r, dst, flags, device):
        s, name = self.s, self.dleq + "_prove"
        off, n = _req_off(req_off)
        (key, ks), (pub, ps), r = _scalar_rows(k, n, s.Ns), _scalar_rows(kA, n, s.Ne), _u8(r, s.Ns)
        B, kB = _elems(B, off, s.Ne), _elems(kB, off, s.Ne)
        if len(r) != n:
            raise ValueError("%s: %d requests, %d rows of randomness" % (name, n, len(r)))
        d, proofs, ok = np.frombuffer(bytes(dst) + b"\0", np.uint8), np.empty((n, 2 * s.Ns), np.uint8), np.empty(n, np.uint8)
        s._call(name, _p(key), ks, _p(pub), ps, _p(B), _p(kB), _p(off), _p(r), _p(d), len(dst), flags, _p(proofs), _p(ok), n, device)
        return proofs, ok

    def verify(self, kA, B, kB, req_off, proofs, dst, flags, device):
        s, name = self.s, self.dleq + "_verify"
        off, n = _req_off(req_off)
        (pub, ps), proofs, B, kB = _scalar_rows(kA, n, s.Ne), _u8(proofs, 2 * s.Ns), _elems(B, off, s.Ne), _elems(kB, off, s.Ne)
        if len(proofs) != n:
            raise ValueError("%s: %d requests, %d proofs" % (name, n, len(proofs)))
        d, ok = np.frombuffer(bytes(dst) + b"\0", np.uint8), np.empty(n, np.uint8)
        s._call(name, _p(pub), ps, _p(B), _p(kB), _p(off), _p(proofs), _p(d), len(dst), flags, _p(ok), n, device)
        return ok

    def poprf_tweak(self, infos, sk, pkS, device):
        s, name = self.s, self.s.oprf + "_poprf_tweak"
        n = len(infos)
        if (sk is None) == (pkS is None):
            raise ValueError("%s: give sk or pkS" % name)
        (ib, io), ok = _blob(infos), np.empty(n, np.uint8)
        key, stride = _scalar_rows(sk, n, s.Ns) if pkS is None else _scalar_rows(pkS, n, s.Ne)
        t, tinv, tw = np.empty((n, s.Ns), np.uint8), np.empty((n, s.Ns), np.uint8), np.empty((n, s.Ne), np.uint8)
        if pkS is None:
            s._call(name, _p(key), stride, None, 0, _p(ib), _p(io), _p(t), _p(tinv), _p(tw), _p(ok), n, device)
            return t, tinv, tw, ok
        s._call(name, None, 0, _p(key), stride, _p(ib), _p(io), None, None, _p(tw), _p(ok), n, device)
        return tw, ok

    def poprf_finalize(self, inputs, infos, blinds, evaluated, device):
        s, name = self.s, self.s.oprf + "_poprf_finalize"
        blinds, evaluated = _u8(blinds, s.Ns), _u8(evaluated, s.Ne)
        n = len(blinds)
        if len(evaluated) != n:
            raise ValueError("%s: %d blinds, %d evaluated elements" % (name, n, len(evaluated)))
        (ib, io), (fb, fo), out, ok = _rag(inputs, n), _rag(infos, n), np.empty((n, s.Nh), np.uint8), np.empty(n, np.uint8)
        s._call(name, _po(ib), _po(io), _po(fb), _po(fo), _p(blinds), _p(evaluated), _p(out), _p(ok), n, device)
        return out, ok

    def poprf_full_evaluate(self, sk, inputs, infos, device):
        s = self.s
        n = len(inputs)
        (key, stride), (ib, io), (fb, fo) = _scalar_rows(sk, n, s.Ns), _blob(inputs), _rag(infos, n)
        out, ok = np.empty((n, s.Nh), np.uint8), np.empty(n, np.uint8)
        s._call(s.oprf + "_poprf_full_evaluate", _p(key), stride, _p(ib), _p(io), _po(fb), _po(fo), _p(out), _p(ok), n, device)
        return out, ok

    def evaluate_verifiable(self, mode, sk, blinded, req_off, r, info, device):
        s = self.s
        if mode not in (OPRF_MODE_VOPRF, OPRF_MODE_POPRF):
            raise ValueError("oprf_evaluate_verifiable: mode 1 or 2")
        off, n = _req_off(req_off)
        blinded = _elems(blinded, off, s.Ne)[:int(off[-1])]
        if mode == OPRF_MODE_VOPRF:
            k = _u8(sk, s.Ns)[:1]
            kA, key_ok = s.scalar_mult(k, None, False, 1, device)
            evaluated, _ = s.evaluate(k, blinded, device) if len(blinded) else (blinded, None)
            B, kB = blinded, evaluated
        else:
            k, tinv, kA, key_ok = self.poprf_tweak([info], sk, None, device)
            evaluated, _ = s.evaluate(tinv, blinded, device) if len(blinded) else (blinded, None)
            B, kB = evaluated, blinded
        proofs, ok = self.prove(k, kA, B, kB, off, r, s.context_string(mode), DLEQ_NO_IDENTITY, device)
        ok &= key_ok[0]
        proofs[ok == 0] = 0
        evaluated = np.array(evaluated, copy=True)
        evaluated[_per_element(off, ok) == 0] = 0
        return evaluated, proofs, ok

    def finalize_verifiable(self, mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info, device):
        s = self.s
        if mode not in (OPRF_MODE_VOPRF, OPRF_MODE_POPRF):
            raise ValueError("oprf_finalize_verifiable: mode 1 or 2")
        off, n = _req_off(req_off)
        n_el = int(off[-1])
        blinded, evaluated = _elems(blinded, off, s.Ne)[:n_el], _elems(evaluated, off, s.Ne)[:n_el]
        blinds = _u8(blinds, s.Ns) if n_el else np.zeros((0, s.Ns), np.uint8)
        if len(inputs) != n_el or len(blinds) != n_el:
            raise ValueError("oprf_finalize_verifiable: %d elements, %d inputs, %d blinds" % (n_el, len(inputs), len(blinds)))
        none = (np.zeros((0, s.Nh), np.uint8), np.zeros(0, np.uint8))
        if mode == OPRF_MODE_VOPRF:
            ok = self.verify(pkS, blinded, evaluated, off, proofs, s.context_string(mode), DLEQ_NO_IDENTITY, device)
            out, item_ok = s.finalize(inputs, blinds, evaluated, device) if n_el else none
        else:
            tweaked, key_ok = self.poprf_tweak([info], None, pkS, device)
            ok = self.verify(tweaked, evaluated, blinded, off, proofs, s.context_string(mode), DLEQ_NO_IDENTITY, device) & key_ok[0]
            out, item_ok = self.poprf_finalize(inputs, [info] * n_el, blinds, evaluated, device) if n_el else none
        failed = np.zeros(n, np.int64)      # elements of each request that finalize refused
        np.add.at(failed, _per_element(off, np.arange(n)), item_ok == 0)
        ok = ok & (failed == 0).astype(np.uint8)
        out = np.array(out, copy=True)
        out[_per_element(off, ok) == 0] = 0
        return out, ok


_R255_DLEQ = _DleqSuite(_R255)


def dleq_prove(k, kA, B, kB, req_off, r, dst, flags=0, device=0):
    """ProveBatchWithRandomnessRFC9497 per request -> (proofs (n_req, 64), ok (n_req,)).  Request g owns element rows req_off[g] .. req_off[g+1]
    of B and kB; k and kA: one row for the call or n_req rows; r: n_req rows drawn by the caller; dst: the caller's tag (0 .. 242 bytes)."""
    return _R255_DLEQ.prove(k, kA, B, kB, req_off, r, dst, flags, device)


def dleq_verify(kA, B, kB, req_off, proofs, dst, flags=0, device=0):
    """VerifyBatchRFC9497 per request -> ok (n_req,), the verdicts"""
    return _R255_DLEQ.verify(kA, B, kB, req_off, proofs, dst, flags, device)


def oprf_poprf_tweak(infos, sk=None, pkS=None, device=0):
    """mode 2.  With sk (secretFromInfo) -> (t, t_inv, t G, ok); with pkS (pointFromInfo) -> (tweaked key, ok).  One key or n rows."""
    return _R255_DLEQ.poprf_tweak(infos, sk, pkS, device)


def oprf_poprf_finalize(inputs, infos, blinds, evaluated, device=0):
    """PartialObliviousClient.Finalize without the proof -> (outputs (n, 64), ok (n,))"""
    return _R255_DLEQ.poprf_finalize(inputs, infos, blinds, evaluated, device)


def oprf_poprf_full_evaluate(sk, inputs, infos, device=0):
    """PartialObliviousServer.FullEvaluate -> (outputs (n, 64), ok (n,)); sk as in oprf_evaluate"""
    return _R255_DLEQ.poprf_full_evaluate(sk, inputs, infos, device)


def oprf_evaluate_verifiable(mode, sk, blinded, req_off, r, info=b"", device=0):
    """VerifiableServer.Evaluate (mode 1) / PartialObliviousServer.Evaluate (mode 2) for n_req requests under ONE key (and one info) ->
    (evaluated (n_elems, 32), proofs (n_req, 64), ok (n_req,)).  r: the proof randomness, one row per request, drawn by the caller.  A request
    with a failed element or proof has ok = 0, a zero proof row and zero evaluated rows."""
    return _R255_DLEQ.evaluate_verifiable(mode, sk, blinded, req_off, r, info, device)


def oprf_finalize_verifiable(mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info=b"", device=0):
    """VerifiableClient.Finalize (mode 1) / PartialObliviousClient.Finalize (mode 2) -> (outputs (n_elems, 64), ok (n_req,)).  The outputs of
    EVERY element of a request whose proof or any element failed are zero."""
    return _R255_DLEQ.finalize_verifiable(mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info, device)


# ---- Ascon AEAD: Ascon128, Ascon128a, Ascon80pq (cipher/ascon/ascon.go) ----
ASCON128, ASCON128A, ASCON80PQ = 1, 2, -1


def ascon_key_size(mode):
    return nat.lib().circl_hip_ascon_key_size(mode)


class AsconCipher:
    """One Ascon mode on host buffers, the reference's Cipher over batches.  key_or_keys: one key (a byte string of the mode's key size:
    the reference's New(key), then many Seal / Open calls) or an (n, key size) array of one key per item.  Nonces are (n, 16); plaintexts,
    ciphertexts and aads are lists of n byte strings (aads None: every item empty)."""
    nonce_size = overhead = 16

    def __init__(self, mode, key_or_keys, device=0):
        self.mode, self.device, self.L = mode, device, nat.lib()
        self.key_size = ascon_key_size(mode)
        if not self.key_size:
            raise ValueError("ascon: mode %r is not served" % (mode,))
        self.shared = isinstance(key_or_keys, (bytes, bytearray))
        if (len(key_or_keys) if self.shared else np.shape(key_or_keys)[-1]) != self.key_size:
            raise ValueError("ascon: a key of this mode has %d bytes" % self.key_size)
        self.keys = _u8(key_or_keys, self.key_size)

    def _rows(self, nonces):
        nonces = _u8(nonces, 16)
        n = nonces.shape[0]
        if not self.shared and self.keys.shape[0] != n:
            raise ValueError("ascon: %d keys, %d nonces" % (self.keys.shape[0], n))
        return nonces, n, 0 if self.shared else self.key_size

    def seal(self, nonces, pts, aads=None):
        """-> the n ciphertexts (ct || tag) as byte strings"""
        nonces, n, stride = self._rows(nonces)
        (pb, po), (ab, ao) = _rag(pts, n), _rag(aads, n)
        ct = np.empty(int(po[n]) + 16 * n, np.uint8)
        nat.check(self.L.circl_hip_ascon_seal(self.mode, _p(self.keys), stride, _p(nonces), _p(pb), _p(po), _po(ab), _po(ao), _p(ct), n, self.device), "ascon_seal")
        return _unrag(ct, po, 16)

    def open(self, nonces, cts, aads=None):
        """-> (the n plaintexts as byte strings, ok (n,)); a ciphertext shorter than a tag is refused here"""
        nonces, n, stride = self._rows(nonces)
        if len(cts) != n or any(len(c) < 16 for c in cts):
            raise ValueError("ascon_open: need %d ciphertexts of at least 16 bytes" % n)
        cb, _ = _blob(cts)
        _, po = _blob([bytes(len(c) - 16) for c in cts])
        ab, ao = _rag(aads, n)
        pt, ok = np.empty(int(po[n]) + 1, np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_ascon_open(self.mode, _p(self.keys), stride, _p(nonces), _p(cb), _p(po), _po(ab), _po(ao), _p(pt), _p(ok), n, self.device),
                  "ascon_open")
        return _unrag(pt, po), ok


# ---- AES-GCM AEAD: AES-128-GCM, AES-256-GCM (hpke/aead.go's AEAD ids 1 and 2; NIST SP 800-38D) ----
AES128GCM, AES256GCM = 16, 32


class AesGcm:
    """AES-GCM on host buffers, Go's cipher.AEAD over batches.  key_or_keys: one key (a byte string of 16 or 32 bytes: one
    cipher.NewGCM, then many Seal / Open calls) or an (n, key size) array of one key per item.  Nonces are (n, 12); with seq (n sequence
    numbers, or one for all) a row is a base nonce and the nonce is row XOR BE96(seq), and one (12,) base nonce may serve the whole batch.
    Plaintexts, ciphertexts and aads are lists of n byte strings (aads None: every item empty).  Distinct (key, nonce) pairs are the
    caller's duty."""
    nonce_size, overhead = 12, 16

    def __init__(self, key_or_keys, device=0):
        self.device, self.L = device, nat.lib()
        self.shared = isinstance(key_or_keys, (bytes, bytearray))
        self.key_size = len(key_or_keys) if self.shared else int(np.shape(key_or_keys)[-1])
        if self.key_size not in (AES128GCM, AES256GCM):
            raise ValueError("aesgcm: a key has 16 or 32 bytes")
        self.keys = _u8(key_or_keys, self.key_size)

    def _rows(self, nonces, seq, n):
        one = seq is not None and (isinstance(nonces, (bytes, bytearray)) or (np.ndim(nonces) == 1 and not isinstance(nonces, (list, tuple))))
        nonces = _u8(nonces, 12)
        if not one and nonces.shape[0] != n or not self.shared and self.keys.shape[0] != n:
            raise ValueError("aesgcm: %d items, %d keys, %d nonces" % (n, self.keys.shape[0], nonces.shape[0]))
        seq = None if seq is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seq, np.uint64), (n,)))
        return nonces, 0 if one else 12, seq, 0 if self.shared else self.key_size

    def seal(self, nonces, pts, aads=None, seq=None):
        """-> the n ciphertexts (ct || tag) as byte strings"""
        n = len(pts)
        nonces, nstride, seq, stride = self._rows(nonces, seq, n)
        (pb, po), (ab, ao) = _rag(pts, n), _rag(aads, n)
        ct = np.empty(int(po[n]) + 16 * n, np.uint8)
        nat.check(self.L.circl_hip_aesgcm_seal(self.key_size, _p(self.keys), stride, _p(nonces), nstride, _po(seq), _p(pb), _p(po), _po(ab), _po(ao), _p(ct), n,
                                               self.device), "aesgcm_seal")
        return _unrag(ct, po, 16)

    def open(self, nonces, cts, aads=None, seq=None):
        """-> (the n plaintexts as byte strings, ok (n,)); a ciphertext shorter than a tag is refused here"""
        n = len(cts)
        if any(len(c) < 16 for c in cts):
            raise ValueError("aesgcm_open: need ciphertexts of at least 16 bytes")
        nonces, nstride, seq, stride = self._rows(nonces, seq, n)
        cb, _ = _blob(cts)
        _, po = _blob([bytes(len(c) - 16) for c in cts])
        ab, ao = _rag(aads, n)
        pt, ok = np.empty(int(po[n]) + 1, np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_aesgcm_open(self.key_size, _p(self.keys), stride, _p(nonces), nstride, _po(seq), _p(cb), _p(po), _po(ab), _po(ao), _p(pt),
                                               _p(ok), n, self.device), "aesgcm_open")
        return _unrag(pt, po), ok


# ---- Prio3Count / Prio3Sum: batch VDAF preparation (vdaf/prio3/count, vdaf/prio3/sum; draft-irtf-cfrg-vdaf-13 section 7) ----
PRIO3_COUNT, PRIO3_SUM = 1, 2


class Prio3:
    """Prio3Count (kind 1, max_measurement 0) or Prio3Sum (kind 2, max_measurement 1 .. 2^63 - 1) over batches of reports on host
    buffers.  shares aggregators (2 .. 255), ctx the application context (at most 255 bytes).  Rows are the reference's MarshalBinary:
    elements of 8 little-endian bytes.  Failed reports have ok = 0 and zero rows."""

    def __init__(self, kind, max_measurement, shares, ctx, device=0):
        self.device, self.L = device, nat.lib()
        self.kind, self.max, self.shares, self.ctx = kind, max_measurement, shares, bytes(ctx)
        self.task = (kind, max_measurement, shares, self.ctx, len(self.ctx))
        self.leader_share_size = self.L.circl_hip_prio3_leader_share_size(kind, max_measurement) if 0 <= max_measurement < 2**64 else 0
        self.prep_share_size = self.L.circl_hip_prio3_prep_share_size(kind)
        self.rand_size = self.L.circl_hip_prio3_rand_size(shares)
        if not (self.leader_share_size and self.prep_share_size and self.rand_size) or len(self.ctx) > 255:
            raise ValueError("prio3: kind 1 (max_measurement 0) or 2 (1 .. 2^63 - 1), 2 .. 255 shares, a context of at most 255 bytes")

    def shard(self, measurements, rand):
        """measurements (n,), rand (n, 32 shares): helpers' seeds then the prove seed -> (leader shares (n, leader_share_size), ok (n,));
        helper j's input share is rand[:, 32 (j - 1) : 32 j]"""
        m, rand = np.ascontiguousarray(measurements, np.uint64), _u8(rand, self.rand_size)
        n = m.shape[0]
        if rand.shape[0] != n:
            raise ValueError("prio3_shard: %d measurements, %d rows of rand" % (n, rand.shape[0]))
        leader, ok = np.empty((n, self.leader_share_size), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_prio3_shard(*self.task, _p(m), _p(rand), _p(leader), _p(ok), n, self.device), "prio3_shard")
        return leader, ok

    def prep_init(self, agg_id, verify_key, nonces, input_shares):
        """input_shares: the leader shares (agg_id 0) or (n, 32) seeds -> (prep shares (n, prep_share_size), out shares (n, 8), ok (n,))"""
        vk, nonces = _u8(verify_key, 32), _u8(nonces, 16)
        shares = _u8(input_shares, self.leader_share_size if agg_id == 0 else 32)
        n = nonces.shape[0]
        if shares.shape[0] != n or vk.shape[0] != 1:
            raise ValueError("prio3_prep_init: %d nonces, %d input shares, %d verify keys" % (n, shares.shape[0], vk.shape[0]))
        prep, out, ok = np.empty((n, self.prep_share_size), np.uint8), np.empty((n, 8), np.uint8), np.empty(n, np.uint8)
        nat.check(self.L.circl_hip_prio3_prep_init(*self.task, agg_id, _p(vk), _p(nonces), _p(shares), _p(prep), _p(out), _p(ok), n, self.device), "prio3_prep_init")
        return prep, out, ok

    def prep_finish(self, prep_shares):
        """PrepSharesToPrep: prep_shares (n, shares, prep_share_size), an item's shares in aggregator order -> ok (n,)"""
        ps = _u8(prep_shares, self.shares * self.prep_share_size)
        ok = np.empty(ps.shape[0], np.uint8)
        nat.check(self.L.circl_hip_prio3_prep_finish(*self.task, _p(ps), _p(ok), ps.shape[0], self.device), "prio3_prep_finish")
        return ok

    def aggregate(self, agg_share, out_shares, mask=None):
        """AggregateUpdate over the batch -> the new aggregate share (8 bytes); mask (n,): only the items where it is not zero"""
        out, agg = _u8(out_shares, 8), _u8(agg_share, 8).copy()
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if mask is not None and mask.shape != (out.shape[0],):
            raise ValueError("prio3_aggregate: a mask has one byte per out share")
        nat.check(self.L.circl_hip_prio3_aggregate(*self.task, _p(out), None if mask is None else _p(mask), _p(agg), out.shape[0], self.device), "prio3_aggregate")
        return agg.tobytes()

    def unshard(self, agg_shares, num_measurements):
        """the aggregate result (an int) from the `shares` aggregate shares; no device is used"""
        a, res = _u8(b"".join(bytes(x) for x in agg_shares), 8), C.c_uint64(0)
        if a.shape[0] != self.shares:
            raise ValueError("prio3_unshard: one aggregate share per aggregator")
        nat.check(self.L.circl_hip_prio3_unshard(*self.task, _p(a), num_measurements, C.byref(res)), "prio3_unshard")
        return res.value
