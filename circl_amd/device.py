"""Device-resident entry points for callers that already hold torch CUDA tensors (bench.py, smoke).

torch is plumbing here: it owns the HBM allocations and the stream; the work is done by the
*_dev functions of the C ABI, launched on torch's current stream.
"""
import ctypes as C

import torch

from . import _native as nat

KEM_SIZES = {512: (800, 1632, 768), 768: (1184, 2400, 1088), 1024: (1568, 3168, 1568)}  # ek, dk, ct
DSA_SIZES = {44: (1312, 2560, 2420), 65: (1952, 4032, 3309), 87: (2592, 4896, 4627),  # pk, sk, sig
             2: (1312, 2528, 2420), 3: (1952, 4000, 3293), 5: (2592, 4864, 4595)}
KERNELS = {"mlkem_hash": 0, "mlkem_encrypt": 1, "mlkem_decrypt": 2, "mlkem_keygen": 3, "mlkem_finish": 4,
           "mldsa_hash": 5, "mldsa_verify": 6, "mldsa_keygen": 7, "mldsa_sign": 8, "mlkem_keytable": 9, "mldsa_keytable": 10, "x25519": 11,
           "ed25519_keygen": 12, "ed25519_sign": 13, "ed25519_verify": 14, "sha512": 15,
           "x448": 16, "ed448_keygen": 17, "ed448_sign": 18, "ed448_verify": 19,
           "frodo_keygen": 20, "frodo_encaps": 21, "frodo_decaps": 22,
           "hpke_x25519": 23, "hpke_x448": 24, "sha256": 25, "hpke_setup": 26, "hpke_aead": 27, "hpke_export": 28,
           "oprf_hash_to_group": 29, "oprf_hash_to_scalar": 30, "oprf_scalar_mult": 31, "oprf_derive_keypair": 32, "oprf_blind": 33, "oprf_evaluate": 34,
           "oprf_finalize": 35, "oprf_full_evaluate": 36, "dleq_composite": 37, "dleq_finish": 38, "oprf_poprf_tweak": 39,
           "oprf_poprf_finalize": 40, "oprf_poprf_full_evaluate": 41}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, cols=None):
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), "need a contiguous uint8 CUDA tensor"
    if cols is not None:
        assert t.shape[-1] == cols, (t.shape, cols)
    return t.data_ptr()


class MLKEMDevice:
    """Holds the output / workspace tensors for one parameter set and batch size."""

    def __init__(self, param, n, device="cuda"):
        self.param, self.n = param, n
        self.EK, self.DK, self.CT = KEM_SIZES[param]
        self.L = nat.lib()
        self.wsb = self.L.circl_hip_mlkem_workspace_size(param, n)
        self.ws = torch.empty(max(self.wsb, 256), dtype=torch.uint8, device=device)
        self.ct = torch.empty((n, self.CT), dtype=torch.uint8, device=device)
        self.ss = torch.empty((n, 32), dtype=torch.uint8, device=device)
        self.status = torch.empty(n, dtype=torch.uint8, device=device)

    def encaps(self, ek, m, ct=None, ss=None, status=None):
        ct = self.ct if ct is None else ct
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_encaps_dev(self.param, _chk(ek, self.EK), _chk(m, 32), _chk(ct, self.CT), _chk(ss, 32),
                                               _chk(status), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_encaps_dev")
        return ct, ss, status

    def encaps_shared(self, ek1, m, ct=None, ss=None, status=None):
        """every item encapsulates to the one key ek1 (a single row)"""
        ct = self.ct if ct is None else ct
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_encaps_shared_dev(self.param, _chk(ek1, self.EK), _chk(m, 32), _chk(ct, self.CT), _chk(ss, 32),
                                                      _chk(status), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_encaps_shared_dev")
        return ct, ss, status

    def encaps_table(self, table, m, key_idx=None, ct=None, ss=None, status=None):
        """through a resident key table (hostapi.KeyTable of kind "mlkem-public"); key_idx None: entry 0 for every item"""
        ct = self.ct if ct is None else ct
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_encaps_table_dev(table.handle, None if key_idx is None else key_idx.data_ptr(), _chk(m, 32), _chk(ct, self.CT),
                                                     _chk(ss, 32), _chk(status), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_encaps_table_dev")
        return ct, ss, status

    def decaps_table(self, table, ct, key_idx=None, ss=None, status=None):
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_decaps_table_dev(table.handle, None if key_idx is None else key_idx.data_ptr(), _chk(ct, self.CT), _chk(ss, 32),
                                                     _chk(status), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_decaps_table_dev")
        return ss, status

    def decaps(self, dk, ct, ss=None, status=None):
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_decaps_dev(self.param, _chk(dk, self.DK), _chk(ct, self.CT), _chk(ss, 32), _chk(status),
                                               self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_decaps_dev")
        return ss, status

    def keygen(self, seeds, ek=None, dk=None):
        if ek is None:
            ek = torch.empty((self.n, self.EK), dtype=torch.uint8, device=seeds.device)
        if dk is None:
            dk = torch.empty((self.n, self.DK), dtype=torch.uint8, device=seeds.device)
        rc = self.L.circl_hip_mlkem_keygen_dev(self.param, _chk(seeds, 64), _chk(ek, self.EK), _chk(dk, self.DK), self.n,
                                               self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_keygen_dev")
        return ek, dk


    def encaps_keyed(self, ek_table, key_idx, m, ct=None, ss=None, status=None):
        """item i encapsulates to row key_idx[i] (int32 / uint32 tensor) of ek_table"""
        ct = self.ct if ct is None else ct
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        nkeys = ek_table.shape[0]
        wsb = self.L.circl_hip_mlkem_keyed_workspace_size(self.param, self.n, nkeys)
        if getattr(self, "_kws", None) is None or self._kws.numel() < wsb:
            self._kws = torch.empty(wsb, dtype=torch.uint8, device=ek_table.device)
        assert key_idx.is_cuda and key_idx.dtype in (torch.int32, torch.uint32) and key_idx.is_contiguous() and key_idx.numel() == self.n
        rc = self.L.circl_hip_mlkem_encaps_keyed_dev(self.param, _chk(ek_table, self.EK), nkeys, key_idx.data_ptr(), _chk(m, 32), _chk(ct, self.CT),
                                                     _chk(ss, 32), _chk(status), self.n, self._kws.data_ptr(), wsb, _stream())
        nat.check(rc, "mlkem_encaps_keyed_dev")
        return ct, ss, status

    def decaps_keyed(self, dk_table, key_idx, ct, ss=None, status=None):
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        nkeys = dk_table.shape[0]
        wsb = self.L.circl_hip_mlkem_keyed_workspace_size(self.param, self.n, nkeys)
        if getattr(self, "_kws", None) is None or self._kws.numel() < wsb:
            self._kws = torch.empty(wsb, dtype=torch.uint8, device=dk_table.device)
        assert key_idx.is_cuda and key_idx.dtype in (torch.int32, torch.uint32) and key_idx.is_contiguous() and key_idx.numel() == self.n
        rc = self.L.circl_hip_mlkem_decaps_keyed_dev(self.param, _chk(dk_table, self.DK), nkeys, key_idx.data_ptr(), _chk(ct, self.CT), _chk(ss, 32),
                                                     _chk(status), self.n, self._kws.data_ptr(), wsb, _stream())
        nat.check(rc, "mlkem_decaps_keyed_dev")
        return ss, status

    def decaps_shared(self, dk1, ct, ss=None, status=None):
        ss = self.ss if ss is None else ss
        status = self.status if status is None else status
        rc = self.L.circl_hip_mlkem_decaps_shared_dev(self.param, _chk(dk1, self.DK), _chk(ct, self.CT), _chk(ss, 32), _chk(status), self.n,
                                                      self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mlkem_decaps_shared_dev")
        return ss, status


class MLDSADevice:
    """Device-resident ML-DSA batch of n items with fixed-length messages (msg_len bytes each) and no contexts:
    the shape of BASELINE.json's ML-DSA configs.  Holds the workspaces and the offset array."""

    def __init__(self, param, n, device="cuda", msg_len=32, nkeys=0, sign=False):
        self.param, self.n, self.msg_len = param, n, msg_len
        self.PK, self.SK, self.SIG = DSA_SIZES[param]
        self.L = nat.lib()
        self.wsb = max(self.L.circl_hip_mldsa_workspace_size(param, n),
                       self.L.circl_hip_mldsa_keyed_workspace_size(param, n, nkeys) if nkeys else 0)
        self.ws = torch.empty(max(self.wsb, 256), dtype=torch.uint8, device=device)
        self.off = torch.arange(0, msg_len * (n + 1), msg_len, dtype=torch.int64, device=device)
        self.ok = torch.empty(n, dtype=torch.uint8, device=device)
        self.sws = None
        if sign:
            self.swsb = self.L.circl_hip_mldsa_sign_workspace_size(param, n)
            self.sws = torch.empty(self.swsb, dtype=torch.uint8, device=device)
            self.rnd0 = torch.zeros((n, 32), dtype=torch.uint8, device=device)

    def _msg(self, msg):
        assert msg.is_cuda and msg.dtype == torch.uint8 and msg.is_contiguous() and msg.numel() >= self.n * self.msg_len + 4, \
            "messages: contiguous uint8 CUDA tensor with >= 4 bytes of slack behind the last one"
        return msg.data_ptr()

    def keygen(self, seeds, pk=None, sk=None):
        pk = torch.empty((self.n, self.PK), dtype=torch.uint8, device=seeds.device) if pk is None else pk
        sk = torch.empty((self.n, self.SK), dtype=torch.uint8, device=seeds.device) if sk is None else sk
        rc = self.L.circl_hip_mldsa_keygen_dev(self.param, _chk(seeds, 32), _chk(pk, self.PK), _chk(sk, self.SK), self.n, self.ws.data_ptr(), self.wsb,
                                               _stream())
        nat.check(rc, "mldsa_keygen_dev")
        return pk, sk

    def sign(self, sk, msg, sig=None, rnd=None, shared=False):
        """deterministic unless rnd (n, 32) is given; asynchronous on the current stream"""
        assert self.sws is not None, "construct with sign=True"
        sig = torch.empty(self.n * self.SIG + 16, dtype=torch.uint8, device=sk.device)[:self.n * self.SIG].view(self.n, self.SIG) if sig is None else sig
        rnd = self.rnd0 if rnd is None else rnd
        fn = self.L.circl_hip_mldsa_sign_shared_dev if shared else self.L.circl_hip_mldsa_sign_dev
        rc = fn(self.param, _chk(sk, self.SK), self._msg(msg), self.off.data_ptr(), None, None, _chk(rnd, 32), 0, _chk(sig, self.SIG), self.n,
                self.sws.data_ptr(), self.swsb, _stream())
        nat.check(rc, "mldsa_sign_dev")
        return sig

    def sign_table(self, table, msg, sig=None, rnd=None):
        """with a private key prepared once (hostapi.KeyTable of kind "mldsa-private")"""
        assert self.sws is not None, "construct with sign=True"
        sig = torch.empty(self.n * self.SIG + 16, dtype=torch.uint8, device=msg.device)[:self.n * self.SIG].view(self.n, self.SIG) if sig is None else sig
        rnd = self.rnd0 if rnd is None else rnd
        rc = self.L.circl_hip_mldsa_sign_table_dev(table.handle, self._msg(msg), self.off.data_ptr(), None, None, _chk(rnd, 32), 0, _chk(sig, self.SIG), self.n,
                                                   self.sws.data_ptr(), self.swsb, _stream())
        nat.check(rc, "mldsa_sign_table_dev")
        return sig

    def verify(self, pk, sig, msg, ok=None):
        ok = self.ok if ok is None else ok
        rc = self.L.circl_hip_mldsa_verify_dev(self.param, _chk(pk, self.PK), _chk(sig, self.SIG), self._msg(msg), self.off.data_ptr(), None, None,
                                               _chk(ok), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mldsa_verify_dev")
        return ok

    def verify_table(self, table, sig, msg, key_idx=None, ok=None):
        """through a resident key table (hostapi.KeyTable of kind "mldsa-public"); key_idx None: entry 0 for every item"""
        ok = self.ok if ok is None else ok
        rc = self.L.circl_hip_mldsa_verify_table_dev(table.handle, None if key_idx is None else key_idx.data_ptr(), _chk(sig, self.SIG), self._msg(msg),
                                                     self.off.data_ptr(), None, None, _chk(ok), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mldsa_verify_table_dev")
        return ok

    def verify_shared(self, pk1, sig, msg, ok=None):
        ok = self.ok if ok is None else ok
        rc = self.L.circl_hip_mldsa_verify_shared_dev(self.param, _chk(pk1, self.PK), _chk(sig, self.SIG), self._msg(msg), self.off.data_ptr(), None, None,
                                                      _chk(ok), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mldsa_verify_shared_dev")
        return ok

    def verify_keyed(self, pk_table, key_idx, sig, msg, ok=None):
        ok = self.ok if ok is None else ok
        nkeys = pk_table.shape[0]
        assert self.L.circl_hip_mldsa_keyed_workspace_size(self.param, self.n, nkeys) <= self.wsb, "construct with nkeys="
        assert key_idx.is_cuda and key_idx.dtype in (torch.int32, torch.uint32) and key_idx.is_contiguous() and key_idx.numel() == self.n
        rc = self.L.circl_hip_mldsa_verify_keyed_dev(self.param, _chk(pk_table, self.PK), nkeys, key_idx.data_ptr(), _chk(sig, self.SIG), self._msg(msg),
                                                     self.off.data_ptr(), None, None, _chk(ok), self.n, self.ws.data_ptr(), self.wsb, _stream())
        nat.check(rc, "mldsa_verify_keyed_dev")
        return ok


def profile_enable(on=True):
    nat.check(nat.lib().circl_hip_profile_enable(int(on)), "profile_enable")


def profile_read(kernel):
    """-> (total_ms, launches) since the last read, for one kernel name of KERNELS."""
    ms, cnt = C.c_double(0), C.c_uint64(0)
    nat.check(nat.lib().circl_hip_profile_read(KERNELS[kernel], C.byref(ms), C.byref(cnt)), "profile_read")
    return ms.value, cnt.value


def valu_probe(device=0, waves_per_simd=4):
    """circl_hip_profile_valu_probe -> (Keccak-round, two-operand integer) wave-instructions per second per SIMD, measured now"""
    k, s = C.c_double(0), C.c_double(0)
    nat.check(nat.lib().circl_hip_profile_valu_probe(device, waves_per_simd, C.byref(k), C.byref(s)), "profile_valu_probe")
    return k.value, s.value


XWING, X25519MLKEM768, KYBER768_X25519, KYBER512_X25519 = 1, 2, 3, 4
KYBER768_X448, KYBER1024_X448 = 5, 6


class HybridDevice:
    """The hybrid KEMs (X-Wing, X25519MLKEM768, Kyber*-X25519, Kyber*-X448) on resident tensors (circl_hip_hybrid_*_dev); every size
    comes from the library.  x25519() / x448() are the bare ladder batches."""

    def __init__(self, scheme, n, device="cuda"):
        self.scheme, self.n = scheme, n
        self.L = nat.lib()
        self.S = {k: getattr(self.L, "circl_hip_hybrid_%s_size" % k)(scheme) for k in ("seed", "eseed", "pk", "sk", "ct", "ss")}
        self.wsb = self.L.circl_hip_hybrid_workspace_size(scheme, n)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=device)
        self.pk = torch.empty((n, self.S["pk"]), dtype=torch.uint8, device=device)
        self.sk = torch.empty((n, self.S["sk"]), dtype=torch.uint8, device=device)
        self.ct = torch.empty((n, self.S["ct"]), dtype=torch.uint8, device=device)
        self.ss = torch.empty((n, self.S["ss"]), dtype=torch.uint8, device=device)
        self.ss2 = torch.empty((n, self.S["ss"]), dtype=torch.uint8, device=device)
        self.status = torch.empty(n, dtype=torch.uint8, device=device)

    def keygen(self, seeds):
        nat.check(self.L.circl_hip_hybrid_keygen_dev(self.scheme, _chk(seeds, self.S["seed"]), _chk(self.pk), _chk(self.sk), self.n,
                                                     self.ws.data_ptr(), self.wsb, _stream()), "hybrid_keygen_dev")
        return self.pk, self.sk

    def encaps(self, pk, eseeds):
        nat.check(self.L.circl_hip_hybrid_encaps_dev(self.scheme, _chk(pk, self.S["pk"]), _chk(eseeds, self.S["eseed"]), _chk(self.ct), _chk(self.ss),
                                                     _chk(self.status), self.n, self.ws.data_ptr(), self.wsb, _stream()), "hybrid_encaps_dev")
        return self.ct, self.ss, self.status

    def decaps(self, sk, ct):
        nat.check(self.L.circl_hip_hybrid_decaps_dev(self.scheme, _chk(sk, self.S["sk"]), _chk(ct, self.S["ct"]), _chk(self.ss2), _chk(self.status),
                                                     self.n, self.ws.data_ptr(), self.wsb, _stream()), "hybrid_decaps_dev")
        return self.ss2, self.status


def x25519(scalar, point=None, out=None, ok=None):
    n = scalar.shape[0]
    out = torch.empty_like(scalar) if out is None else out
    ok = torch.empty(n, dtype=torch.uint8, device=scalar.device) if ok is None else ok
    nat.check(nat.lib().circl_hip_x25519_dev(_chk(scalar, 32), None if point is None else _chk(point, 32), _chk(out, 32), _chk(ok), n, _stream()),
              "x25519_dev")
    return out, ok


def x448(scalar, point=None, out=None, ok=None):
    """circl_hip_x448_dev on (n, 56) tensors: Shared(scalar_i, point_i), or KeyGen(scalar_i) when point is None -> (out, ok)"""
    n = scalar.shape[0]
    out = torch.empty_like(scalar) if out is None else out
    ok = torch.empty(n, dtype=torch.uint8, device=scalar.device) if ok is None else ok
    nat.check(nat.lib().circl_hip_x448_dev(_chk(scalar, 56), None if point is None else _chk(point, 56), _chk(out, 56), _chk(ok), n, _stream()),
              "x448_dev")
    return out, ok


class FrodoDevice:
    """FrodoKEM-640-SHAKE on resident tensors (circl_hip_frodo640shake_*_dev), on torch's current stream."""
    PK, SK, CT, SS, SEED, ESEED = 9616, 19888, 9720, 16, 48, 16

    def __init__(self, n, device="cuda"):
        self.n = n
        self.L = nat.lib()
        self.wsb = self.L.circl_hip_frodo640shake_workspace_size(n)
        self.ws = torch.empty(max(self.wsb, 256), dtype=torch.uint8, device=device)
        self.pk = torch.empty((n, self.PK), dtype=torch.uint8, device=device)
        self.sk = torch.empty((n, self.SK), dtype=torch.uint8, device=device)
        self.ct = torch.empty((n, self.CT), dtype=torch.uint8, device=device)
        self.ss = torch.empty((n, self.SS), dtype=torch.uint8, device=device)
        self.ss2 = torch.empty((n, self.SS), dtype=torch.uint8, device=device)

    def keygen(self, seeds):
        nat.check(self.L.circl_hip_frodo640shake_keygen_dev(_chk(seeds, self.SEED), _chk(self.pk), _chk(self.sk), self.n, self.ws.data_ptr(), self.wsb,
                                                            _stream()), "frodo640shake_keygen_dev")
        return self.pk, self.sk

    def encaps(self, pk, eseeds):
        nat.check(self.L.circl_hip_frodo640shake_encaps_dev(_chk(pk, self.PK), _chk(eseeds, self.ESEED), _chk(self.ct), _chk(self.ss), self.n,
                                                            self.ws.data_ptr(), self.wsb, _stream()), "frodo640shake_encaps_dev")
        return self.ct, self.ss

    def decaps(self, sk, ct):
        nat.check(self.L.circl_hip_frodo640shake_decaps_dev(_chk(sk, self.SK), _chk(ct, self.CT), _chk(self.ss2), self.n, self.ws.data_ptr(), self.wsb,
                                                            _stream()), "frodo640shake_decaps_dev")
        return self.ss2


HPKE_KEM_X25519_HKDF_SHA256, HPKE_KEM_X448_HKDF_SHA512 = 0x20, 0x21


class HpkeDhkemDevice:
    """HPKE DHKEM over X25519 (kem = 0x20) or X448 (0x21) on resident tensors (circl_hip_hpke_dhkem_*_dev), on torch's current stream.
    Key rows are (n, N) with N = 32 / 56, shared secrets (n, S) with S = 32 / 64; every call returns new tensors unless given."""

    def __init__(self, kem, device="cuda"):
        self.kem, self.device = kem, device
        self.L = nat.lib()
        self.N, self.S = self.L.circl_hip_hpke_dhkem_key_size(kem), self.L.circl_hip_hpke_dhkem_ss_size(kem)
        if not self.N:
            raise ValueError("unknown HPKE KEM id 0x%x" % kem)

    def _out(self, n, cols=None):
        return torch.empty(n if cols is None else (n, cols), dtype=torch.uint8, device=self.device)

    def _opt(self, t):
        return None if t is None else _chk(t, self.N)

    def derive_keypair(self, ikm, sk=None, pk=None):
        n = ikm.shape[0]
        sk = self._out(n, self.N) if sk is None else sk
        pk = self._out(n, self.N) if pk is None else pk
        nat.check(self.L.circl_hip_hpke_dhkem_derive_keypair_dev(self.kem, _chk(ikm, self.N), _chk(sk, self.N), _chk(pk, self.N), n, _stream()),
                  "hpke_dhkem_derive_keypair_dev")
        return sk, pk

    def encap(self, pkR, ikmE, enc=None, ss=None, ok=None):
        n = pkR.shape[0]
        enc, ss, ok = (self._out(n, self.N) if enc is None else enc, self._out(n, self.S) if ss is None else ss, self._out(n) if ok is None else ok)
        nat.check(self.L.circl_hip_hpke_dhkem_encap_dev(self.kem, _chk(pkR, self.N), _chk(ikmE, self.N), _chk(enc, self.N), _chk(ss, self.S), _chk(ok), n,
                                                        _stream()), "hpke_dhkem_encap_dev")
        return enc, ss, ok

    def decap(self, skR, enc, pkR=None, ss=None, ok=None):
        n = skR.shape[0]
        ss, ok = self._out(n, self.S) if ss is None else ss, self._out(n) if ok is None else ok
        nat.check(self.L.circl_hip_hpke_dhkem_decap_dev(self.kem, _chk(skR, self.N), self._opt(pkR), _chk(enc, self.N), _chk(ss, self.S), _chk(ok), n,
                                                        _stream()), "hpke_dhkem_decap_dev")
        return ss, ok

    def auth_encap(self, pkR, skS, ikmE, pkS=None, enc=None, ss=None, ok=None):
        n = pkR.shape[0]
        enc, ss, ok = (self._out(n, self.N) if enc is None else enc, self._out(n, self.S) if ss is None else ss, self._out(n) if ok is None else ok)
        nat.check(self.L.circl_hip_hpke_dhkem_auth_encap_dev(self.kem, _chk(pkR, self.N), _chk(skS, self.N), self._opt(pkS), _chk(ikmE, self.N),
                                                             _chk(enc, self.N), _chk(ss, self.S), _chk(ok), n, _stream()), "hpke_dhkem_auth_encap_dev")
        return enc, ss, ok

    def auth_decap(self, skR, enc, pkS, pkR=None, ss=None, ok=None):
        n = skR.shape[0]
        ss, ok = self._out(n, self.S) if ss is None else ss, self._out(n) if ok is None else ok
        nat.check(self.L.circl_hip_hpke_dhkem_auth_decap_dev(self.kem, _chk(skR, self.N), self._opt(pkR), _chk(enc, self.N), _chk(pkS, self.N),
                                                             _chk(ss, self.S), _chk(ok), n, _stream()), "hpke_dhkem_auth_decap_dev")
        return ss, ok


class Ragged:
    """n byte strings on the device: blob (uint8) and the n + 1 offsets (int64 tensor holding the uint64 values).  None stands for
    'every item empty' wherever a Ragged is expected."""

    def __init__(self, items, device="cuda"):
        import numpy as np
        off = np.zeros(len(items) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in items])
        self.lens = [len(x) for x in items]
        self.off_host = off
        self.blob = torch.from_numpy(np.frombuffer(b"".join(bytes(x) for x in items) + bytes(16), np.uint8).copy()).to(device)
        self.off = torch.from_numpy(off).to(device)

    def args(self):
        return self.blob.data_ptr(), self.off.data_ptr()


def _rag_args(r):
    return (None, None) if r is None else r.args()


class HpkeSuiteDevice:
    """One HPKE suite (kem, kdf, aead) on resident tensors (circl_hip_hpke_*_dev), on torch's current stream.  Key rows are (n, N), context
    rows (n, CS); ragged inputs are Ragged objects (or None).  Ciphertexts / plaintexts are flat uint8 tensors laid out by the plaintext
    offsets: item i's ciphertext is at pt_off[i] + 16 i."""

    def __init__(self, kem, kdf, aead, device="cuda"):
        self.kem, self.kdf, self.aead, self.device = kem, kdf, aead, device
        self.L = nat.lib()
        self.N, self.CS = self.L.circl_hip_hpke_dhkem_key_size(kem), self.L.circl_hip_hpke_context_size(kdf)
        if not self.N or not self.CS:
            raise ValueError("HPKE suite (0x%x, 0x%x, 0x%x) is not served" % (kem, kdf, aead))

    def _out(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def _row(self, t):
        return None if t is None else _chk(t, self.N)

    def _setup(self, mode, rows, info, psk, psk_id):
        return [self.kem, self.kdf, self.aead, mode] + [self._row(r) for r in rows] + [*_rag_args(info), *_rag_args(psk), *_rag_args(psk_id)]

    def setup_sender(self, mode, pkR, ikmE, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        n = pkR.shape[0]
        enc, ctx, ok = self._out(n, self.N), self._out(n, self.CS), self._out(n)
        nat.check(self.L.circl_hip_hpke_setup_sender_dev(*self._setup(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id), _chk(enc), _chk(ctx), _chk(ok), n,
                                                         _stream()), "hpke_setup_sender_dev")
        return enc, ctx, ok

    def setup_receiver(self, mode, skR, enc, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        n = skR.shape[0]
        ctx, ok = self._out(n, self.CS), self._out(n)
        nat.check(self.L.circl_hip_hpke_setup_receiver_dev(*self._setup(mode, (skR, pkR, enc, pkS), info, psk, psk_id), _chk(ctx), _chk(ok), n, _stream()),
                  "hpke_setup_receiver_dev")
        return ctx, ok

    def seal(self, ctx, pt, aad=None, seq=None):
        """pt: Ragged; seq: int64 tensor holding the uint64 sequence numbers, or None -> flat ciphertext tensor"""
        n = ctx.shape[0]
        ct = self._out(int(pt.off_host[n]) + 16 * n)
        nat.check(self.L.circl_hip_hpke_seal_dev(self.aead, _chk(ctx, self.CS), self.CS, None if seq is None else seq.data_ptr(), *pt.args(), *_rag_args(aad),
                                                 _chk(ct), n, _stream()), "hpke_seal_dev")
        return ct

    def open(self, ctx, ct, pt_off, aad=None, seq=None):
        """ct: flat tensor; pt_off: Ragged giving the plaintext layout (its blob is not read) -> (flat plaintext tensor, ok)"""
        n = ctx.shape[0]
        pt, ok = self._out(int(pt_off.off_host[n]) + 1), self._out(n)
        nat.check(self.L.circl_hip_hpke_open_dev(self.aead, _chk(ctx, self.CS), self.CS, None if seq is None else seq.data_ptr(), _chk(ct), pt_off.off.data_ptr(),
                                                 *_rag_args(aad), _chk(pt), _chk(ok), n, _stream()), "hpke_open_dev")
        return pt, ok

    def export(self, ctx, exporter_context, length):
        n = ctx.shape[0]
        out = self._out(n, length)
        nat.check(self.L.circl_hip_hpke_export_dev(self.kdf, self.kem, self.aead, _chk(ctx, self.CS), self.CS, *_rag_args(exporter_context), length, _chk(out), n,
                                                   _stream()), "hpke_export_dev")
        return out

    def seal_single(self, mode, pkR, ikmE, pt, aad=None, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        n = pkR.shape[0]
        enc, ct, ok = self._out(n, self.N), self._out(int(pt.off_host[n]) + 16 * n), self._out(n)
        nat.check(self.L.circl_hip_hpke_seal_single_dev(*self._setup(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id), *pt.args(), *_rag_args(aad), _chk(enc),
                                                        _chk(ct), _chk(ok), n, _stream()), "hpke_seal_single_dev")
        return enc, ct, ok

    def open_single(self, mode, skR, enc, ct, pt_off, aad=None, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        n = skR.shape[0]
        pt, ok = self._out(int(pt_off.off_host[n]) + 1), self._out(n)
        nat.check(self.L.circl_hip_hpke_open_single_dev(*self._setup(mode, (skR, pkR, enc, pkS), info, psk, psk_id), _chk(ct), pt_off.off.data_ptr(),
                                                        *_rag_args(aad), _chk(pt), _chk(ok), n, _stream()), "hpke_open_single_dev")
        return pt, ok

    def export_single(self, mode, pkR, ikmE, exporter_context, length, info=None, psk=None, psk_id=None, skS=None, pkS=None):
        n = pkR.shape[0]
        enc, out, ok = self._out(n, self.N), self._out(n, length), self._out(n)
        nat.check(self.L.circl_hip_hpke_export_single_dev(*self._setup(mode, (pkR, ikmE, skS, pkS), info, psk, psk_id), *_rag_args(exporter_context), length,
                                                          _chk(enc), _chk(out), _chk(ok), n, _stream()), "hpke_export_single_dev")
        return enc, out, ok

    def export_single_receiver(self, mode, skR, enc, exporter_context, length, info=None, psk=None, psk_id=None, pkS=None, pkR=None):
        n = skR.shape[0]
        out, ok = self._out(n, length), self._out(n)
        nat.check(self.L.circl_hip_hpke_export_single_receiver_dev(*self._setup(mode, (skR, pkR, enc, pkS), info, psk, psk_id), *_rag_args(exporter_context),
                                                                   length, _chk(out), _chk(ok), n, _stream()), "hpke_export_single_receiver_dev")
        return out, ok


class _OprfGroupDevice:
    """The group operations and the proof-free part of OPRF for one suite on resident tensors, on torch's current stream, written once:
    OprfDevice and NistpOprfDevice bind it.  _group / _oprf: the prefixes of the symbols (and of the names in error messages); _lead: the
    arguments every call starts with (the curve id, or none); Ns / Ne / Nh: bytes of a scalar, an element, an output; _nonuniform:
    hash_to_group takes a flags argument."""

    def _out(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def _scalars(self, t, n):
        """(pointer, stride) of n scalar rows, or of one row shared by the batch"""
        shared = t.numel() == self.Ns and n != 1
        assert shared or t.shape == (n, self.Ns), (t.shape, n)
        return _chk(t, self.Ns), 0 if shared else self.Ns

    def _call(self, name, *args):
        nat.check(getattr(self.L, "circl_hip_" + name)(*self._lead, *args, _stream()), name)

    def _hash(self, name, width, msgs, n, dst, flags=()):
        import numpy as np
        d = np.frombuffer(bytes(dst) + b"\0", np.uint8)      # the tag is host bytes in both forms
        out = self._out(n, width)
        self._call(self._group + name, *_rag_args(msgs), d.ctypes.data_as(C.c_void_p), len(dst), *flags, _chk(out), n)
        return out

    def hash_to_group(self, msgs, n, dst, nonuniform=False):
        return self._hash("_hash_to_group_dev", self.Ne, msgs, n, dst, (1 if nonuniform else 0,) if self._nonuniform else ())

    def hash_to_scalar(self, msgs, n, dst):
        return self._hash("_hash_to_scalar_dev", self.Ns, msgs, n, dst)

    def scalar_mult(self, scalars, elems=None, invert=False, n=None):
        n = elems.shape[0] if elems is not None else (scalars.shape[0] if n is None else n)
        out, ok = self._out(n, self.Ne), self._out(n)
        self._call(self._group + "_scalar_mult_dev", *self._scalars(scalars, n), None if elems is None else _chk(elems, self.Ne), 1 if invert else 0,
                   _chk(out), _chk(ok), n)
        return out, ok

    def derive_keypair(self, mode, seeds, infos=None):
        n = seeds.shape[0]
        sk, pk, ok = self._out(n, self.Ns), self._out(n, self.Ne), self._out(n)
        self._call(self._oprf + "_derive_keypair_dev", mode, _chk(seeds, 32), *_rag_args(infos), _chk(sk), _chk(pk), _chk(ok), n)
        return sk, pk, ok

    def blind(self, mode, inputs, blinds):
        n = blinds.shape[0]
        out, ok = self._out(n, self.Ne), self._out(n)
        self._call(self._oprf + "_blind_dev", mode, *_rag_args(inputs), _chk(blinds, self.Ns), _chk(out), _chk(ok), n)
        return out, ok

    def evaluate(self, sk, blinded):
        n = blinded.shape[0]
        out, ok = self._out(n, self.Ne), self._out(n)
        self._call(self._oprf + "_evaluate_dev", *self._scalars(sk, n), _chk(blinded, self.Ne), _chk(out), _chk(ok), n)
        return out, ok

    def finalize(self, inputs, blinds, evaluated):
        n = blinds.shape[0]
        out, ok = self._out(n, self.Nh), self._out(n)
        self._call(self._oprf + "_finalize_dev", *_rag_args(inputs), _chk(blinds, self.Ns), _chk(evaluated, self.Ne), _chk(out), _chk(ok), n)
        return out, ok

    def full_evaluate(self, mode, sk, inputs, n):
        out, ok = self._out(n, self.Nh), self._out(n)
        self._call(self._oprf + "_full_evaluate_dev", mode, *self._scalars(sk, n), *_rag_args(inputs), _chk(out), _chk(ok), n)
        return out, ok

    # ---- batch DLEQ proofs and the verifiable modes (circl_hip_[nistp_]dleq_*_dev, circl_hip_oprf_[nistp_]poprf_*_dev) ----
    # _dleq_sym: the prefix of the proofs' symbols; _tail: the end of the context string; a proof is a row of 2 Ns bytes
    def _ctx(self, mode):
        return b"OPRFV1-" + bytes([mode]) + self._tail

    def _elem_rows(self, t, n):
        """(pointer, stride) of n element rows (public keys), or of one row shared by the batch"""
        shared = t.numel() == self.Ne and n != 1
        assert shared or t.shape == (n, self.Ne), (t.shape, n)
        return _chk(t, self.Ne), 0 if shared else self.Ne

    def _requests(self, req_off):
        """(offsets on the device as an int64 tensor, n_req, n_elems, elements per request as a device tensor) of host offsets"""
        import numpy as np
        off = np.ascontiguousarray(req_off, dtype=np.int64)
        off_d = torch.from_numpy(off).to(self.device)
        return off_d, len(off) - 1, int(off[-1] - off[0]), off_d[1:] - off_d[:-1]

    def _dleq(self, verify, k, kA, B, kB, req_off, r, proofs, dst, flags):
        import numpy as np
        off_d, n, n_el, _ = self._requests(req_off)
        d = np.frombuffer(bytes(dst) + b"\0", np.uint8)
        wsb = getattr(self.L, "circl_hip_" + self._dleq_sym + "_workspace_size")(*self._lead, n, n_el)
        ws, ok = self._out(max(wsb, 256)), self._out(n)
        tail = (d.ctypes.data_as(C.c_void_p), len(dst), flags)
        common = (*self._elem_rows(kA, n), _chk(B, self.Ne), _chk(kB, self.Ne), off_d.data_ptr())
        if verify:
            self._call(self._dleq_sym + "_verify_dev", *common, _chk(proofs, 2 * self.Ns), *tail, _chk(ok), n, n_el, _chk(ws), wsb)
            return ok
        proofs = self._out(n, 2 * self.Ns)
        self._call(self._dleq_sym + "_prove_dev", *self._scalars(k, n), *common, _chk(r, self.Ns), *tail, _chk(proofs), _chk(ok), n, n_el, _chk(ws), wsb)
        return proofs, ok

    def dleq_prove(self, k, kA, B, kB, req_off, r, dst, flags=0):
        """req_off: n_req + 1 HOST offsets in elements -> (proofs (n_req, 2 Ns), ok (n_req,))"""
        return self._dleq(False, k, kA, B, kB, req_off, r, None, dst, flags)

    def dleq_verify(self, kA, B, kB, req_off, proofs, dst, flags=0):
        return self._dleq(True, None, kA, B, kB, req_off, None, proofs, dst, flags)

    def poprf_tweak(self, infos, n, sk=None, pkS=None):
        """with sk -> (t, t_inv, t G, ok); with pkS -> (tweaked key, ok)"""
        assert (sk is None) != (pkS is None)
        t, tinv, tw, ok = self._out(n, self.Ns), self._out(n, self.Ns), self._out(n, self.Ne), self._out(n)
        if pkS is None:
            self._call(self._oprf + "_poprf_tweak_dev", *self._scalars(sk, n), None, 0, *_rag_args(infos), _chk(t), _chk(tinv), _chk(tw), _chk(ok), n)
            return t, tinv, tw, ok
        self._call(self._oprf + "_poprf_tweak_dev", None, 0, *self._elem_rows(pkS, n), *_rag_args(infos), None, None, _chk(tw), _chk(ok), n)
        return tw, ok

    def poprf_finalize(self, inputs, infos, blinds, evaluated):
        n = blinds.shape[0]
        out, ok = self._out(n, self.Nh), self._out(n)
        self._call(self._oprf + "_poprf_finalize_dev", *_rag_args(inputs), *_rag_args(infos), _chk(blinds, self.Ns), _chk(evaluated, self.Ne), _chk(out), _chk(ok), n)
        return out, ok

    def poprf_full_evaluate(self, sk, inputs, infos, n):
        out, ok = self._out(n, self.Nh), self._out(n)
        self._call(self._oprf + "_poprf_full_evaluate_dev", *self._scalars(sk, n), *_rag_args(inputs), *_rag_args(infos), _chk(out), _chk(ok), n)
        return out, ok

    def evaluate_verifiable(self, mode, sk, blinded, req_off, r, info=b""):
        """The verifiable server's Evaluate of modes 1 and 2 for n_req requests under one key (and one info) -> (evaluated, proofs, ok per
        request); a failed request has a zero proof row and zero evaluated rows."""
        assert mode in (1, 2)
        _, n, n_el, counts = self._requests(req_off)
        if mode == 1:
            k = sk.reshape(1, self.Ns)
            kA, key_ok = self.scalar_mult(k, n=1)
            evaluated, _ = self.evaluate(k, blinded)
            B, kB = blinded, evaluated
        else:
            k, tinv, kA, key_ok = self.poprf_tweak(Ragged([info], self.device), 1, sk=sk.reshape(1, self.Ns))
            evaluated, _ = self.evaluate(tinv, blinded)
            B, kB = evaluated, blinded
        proofs, ok = self.dleq_prove(k, kA, B, kB, req_off, r, self._ctx(mode), 1)
        ok = ok & key_ok[0]
        proofs = proofs * ok[:, None]
        return evaluated * torch.repeat_interleave(ok, counts)[:, None], proofs, ok

    def finalize_verifiable(self, mode, pkS, inputs, blinds, blinded, evaluated, req_off, proofs, info=b""):
        """The verifiable client's Finalize of modes 1 and 2 -> (outputs (n_elems, Nh), ok per request); the outputs of EVERY element of a request
        whose proof or any element failed are zero.  inputs: a Ragged of n_elems items."""
        assert mode in (1, 2)
        off_d, n, n_el, counts = self._requests(req_off)
        shared = lambda t: t.reshape(1, self.Ne)
        if mode == 1:
            ok = self.dleq_verify(shared(pkS), blinded, evaluated, req_off, proofs, self._ctx(mode), 1)
            out, item_ok = self.finalize(inputs, blinds, evaluated)
        else:
            tweaked, key_ok = self.poprf_tweak(Ragged([info], self.device), 1, pkS=pkS.reshape(1, self.Ne))
            ok = self.dleq_verify(shared(tweaked), evaluated, blinded, req_off, proofs, self._ctx(mode), 1) & key_ok[0]
            out, item_ok = self.poprf_finalize(inputs, Ragged([info] * n_el, self.device), blinds, evaluated)
        failed = torch.zeros(n, dtype=torch.int64, device=self.device)
        failed.index_add_(0, torch.repeat_interleave(torch.arange(n, device=self.device), counts), (item_ok == 0).to(torch.int64))
        ok = ok & (failed == 0).to(torch.uint8)
        return out * torch.repeat_interleave(ok, counts)[:, None], ok


class OprfDevice(_OprfGroupDevice):
    """ristretto255 and base-mode OPRF (suite ristretto255-SHA512) on resident tensors (circl_hip_ristretto255_*_dev, circl_hip_oprf_*_dev),
    on torch's current stream.  Elements, scalars, keys and blinds are (n, 32) uint8 tensors, OPRF outputs (n, 64); ragged inputs are Ragged
    objects (or None: every item empty).  A key or scalar of shape (32,) or (1, 32) is shared by the batch.  Failed items have ok = 0 and zero
    rows."""
    _group, _oprf, _dleq_sym, _lead, _nonuniform, Ns, Ne, Nh, _tail = "ristretto255", "oprf", "dleq", (), False, 32, 32, 64, b"-ristretto255-SHA512"

    def __init__(self, device="cuda"):
        self.device = device
        self.L = nat.lib()

    def hash_to_group(self, msgs, n, dst):
        return super().hash_to_group(msgs, n, dst)


class AsconCipherDevice:
    """One Ascon mode on resident tensors (circl_hip_ascon_*_dev), on torch's current stream.  keys: a (key size,) tensor (one key for
    every item) or (n, key size); nonces (n, 16); ragged inputs are Ragged objects (aad None: every item empty).  Ciphertexts / plaintexts
    are flat uint8 tensors laid out by the plaintext offsets: item i's ciphertext is at pt_off[i] + 16 i."""

    def __init__(self, mode, keys, device="cuda"):
        self.mode, self.device, self.L = mode, device, nat.lib()
        self.KS = self.L.circl_hip_ascon_key_size(mode)
        if not self.KS:
            raise ValueError("ascon: mode %r is not served" % (mode,))
        self.keys, self.stride = keys, 0 if keys.dim() == 1 else self.KS
        _chk(keys, self.KS)

    def _out(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def seal(self, nonces, pt, aad=None):
        """pt: Ragged -> flat ciphertext tensor"""
        n = nonces.shape[0]
        ct = self._out(int(pt.off_host[n]) + 16 * n)
        nat.check(self.L.circl_hip_ascon_seal_dev(self.mode, _chk(self.keys), self.stride, _chk(nonces, 16), *pt.args(), *_rag_args(aad), _chk(ct), n, _stream()),
                  "ascon_seal_dev")
        return ct

    def open(self, nonces, ct, pt_off, aad=None):
        """ct: flat tensor; pt_off: Ragged giving the plaintext layout (its blob is not read) -> (flat plaintext tensor, ok)"""
        n = nonces.shape[0]
        pt, ok = self._out(int(pt_off.off_host[n]) + 1), self._out(n)
        nat.check(self.L.circl_hip_ascon_open_dev(self.mode, _chk(self.keys), self.stride, _chk(nonces, 16), _chk(ct), pt_off.off.data_ptr(), *_rag_args(aad),
                                                  _chk(pt), _chk(ok), n, _stream()), "ascon_open_dev")
        return pt, ok


class AesGcmDevice:
    """AES-128-GCM / AES-256-GCM on resident tensors (circl_hip_aesgcm_*_dev), on torch's current stream.  keys: a (16,) / (32,) tensor
    (one key for every item) or (n, key size); nonces (n, 12), or with seq (an (n,) int64 / uint64 tensor of sequence numbers) base nonces,
    (n, 12) or one (12,) for the batch; ragged inputs are Ragged objects (aad None: every item empty).  Ciphertexts / plaintexts are flat
    uint8 tensors laid out by the plaintext offsets: item i's ciphertext is at pt_off[i] + 16 i.  Distinct (key, nonce) pairs are the
    caller's duty."""

    def __init__(self, keys, device="cuda"):
        self.device, self.L = device, nat.lib()
        self.KS = int(keys.shape[-1])
        if self.KS not in (16, 32):
            raise ValueError("aesgcm: a key has 16 or 32 bytes")
        self.keys, self.stride = keys, 0 if keys.dim() == 1 else self.KS
        _chk(keys, self.KS)

    def _out(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def _nonce(self, nonces, seq):
        if nonces.dim() == 1 and seq is None:
            raise ValueError("aesgcm: one base nonce for the batch needs seq")
        return _chk(nonces, 12), 0 if nonces.dim() == 1 else 12, None if seq is None else seq.data_ptr()

    def seal(self, nonces, pt, aad=None, seq=None):
        """pt: Ragged -> flat ciphertext tensor"""
        n = pt.off_host.shape[0] - 1
        ct = self._out(int(pt.off_host[n]) + 16 * n)
        nat.check(self.L.circl_hip_aesgcm_seal_dev(self.KS, _chk(self.keys), self.stride, *self._nonce(nonces, seq), *pt.args(), *_rag_args(aad), _chk(ct), n,
                                                   _stream()), "aesgcm_seal_dev")
        return ct

    def open(self, nonces, ct, pt_off, aad=None, seq=None):
        """ct: flat tensor; pt_off: Ragged giving the plaintext layout (its blob is not read) -> (flat plaintext tensor, ok)"""
        n = pt_off.off_host.shape[0] - 1
        pt, ok = self._out(int(pt_off.off_host[n]) + 1), self._out(n)
        nat.check(self.L.circl_hip_aesgcm_open_dev(self.KS, _chk(self.keys), self.stride, *self._nonce(nonces, seq), _chk(ct), pt_off.off.data_ptr(),
                                                   *_rag_args(aad), _chk(pt), _chk(ok), n, _stream()), "aesgcm_open_dev")
        return pt, ok


class NistpOprfDevice(_OprfGroupDevice):
    """P-256 / P-384 and base-mode OPRF on them (suites P256-SHA256, P384-SHA384) on resident tensors (circl_hip_nistp_*_dev,
    circl_hip_oprf_nistp_*_dev), on torch's current stream; shaped like OprfDevice.  curve = 256 or 384.  Scalars, keys and blinds are (n, Ns)
    big-endian rows (Ns = 32 / 48), elements (n, Ne) SEC 1 compressed rows (Ne = 33 / 49; the identity: the zero row), seeds (n, 32), OPRF
    outputs (n, Nh = Ns); ragged inputs are Ragged objects (or None: every item empty).  A key or scalar of shape (Ns,) or (1, Ns) is shared
    by the batch.  Failed items have ok = 0 and zero rows."""
    _group, _oprf, _dleq_sym, _nonuniform = "nistp", "oprf_nistp", "nistp_dleq", True

    def __init__(self, curve, device="cuda"):
        if curve not in (256, 384):
            raise ValueError("curve is 256 or 384")
        self.curve, self.device, self.L, self._lead = curve, device, nat.lib(), (curve,)
        self.Ns = curve // 8
        self.Ne, self.Nh = self.Ns + 1, self.Ns
        self._tail = b"-P256-SHA256" if curve == 256 else b"-P384-SHA384"


class Prio3Device:
    """Prio3Count / Prio3Sum on resident tensors (circl_hip_prio3_*_dev), on torch's current stream; shaped like hostapi.Prio3.  Measurements
    are an (n,) int64 / uint64 tensor, every other array a contiguous uint8 tensor whose storage is 8-byte aligned; the verify key is a
    (32,) tensor, the aggregate share an (8,) tensor that aggregate() updates in place.  The workspace grows to the largest batch seen
    and holds the last call's per-report state, as secret as its inputs."""

    def __init__(self, kind, max_measurement, shares, ctx, device="cuda"):
        self.device, self.L = device, nat.lib()
        self.kind, self.max, self.shares, self.ctx = kind, max_measurement, shares, bytes(ctx)
        self.task = (kind, max_measurement, shares, self.ctx, len(self.ctx))
        self.leader_share_size = self.L.circl_hip_prio3_leader_share_size(kind, max_measurement) if 0 <= max_measurement < 2**64 else 0
        self.prep_share_size = self.L.circl_hip_prio3_prep_share_size(kind)
        self.rand_size = self.L.circl_hip_prio3_rand_size(shares)
        if not (self.leader_share_size and self.prep_share_size and self.rand_size) or len(self.ctx) > 255:
            raise ValueError("prio3: kind 1 (max_measurement 0) or 2 (1 .. 2^63 - 1), 2 .. 255 shares, a context of at most 255 bytes")
        self.ws = None

    def _out(self, *shape):
        return torch.empty(shape, dtype=torch.uint8, device=self.device)

    def _ws(self, n):
        need = self.L.circl_hip_prio3_workspace_size(self.kind, self.max, n)
        if self.ws is None or self.ws.numel() < need:
            self.ws = self._out(need)
        return self.ws.data_ptr(), self.ws.numel()

    def shard(self, measurements, rand):
        n = measurements.shape[0]
        assert measurements.is_cuda and measurements.element_size() == 8 and measurements.is_contiguous()
        leader, ok = self._out(n, self.leader_share_size), self._out(n)
        nat.check(self.L.circl_hip_prio3_shard_dev(*self.task, measurements.data_ptr(), _chk(rand, self.rand_size), _chk(leader), _chk(ok), n, *self._ws(n), _stream()),
                  "prio3_shard_dev")
        return leader, ok

    def prep_init(self, agg_id, verify_key, nonces, input_shares):
        n = nonces.shape[0]
        prep, out, ok = self._out(n, self.prep_share_size), self._out(n, 8), self._out(n)
        nat.check(self.L.circl_hip_prio3_prep_init_dev(*self.task, agg_id, _chk(verify_key, 32), _chk(nonces, 16),
                                                       _chk(input_shares, self.leader_share_size if agg_id == 0 else 32), _chk(prep), _chk(out), _chk(ok), n,
                                                       *self._ws(n), _stream()), "prio3_prep_init_dev")
        return prep, out, ok

    def prep_finish(self, prep_shares):
        n = prep_shares.shape[0]
        ok = self._out(n)
        nat.check(self.L.circl_hip_prio3_prep_finish_dev(*self.task, _chk(prep_shares), _chk(ok), n, _stream()), "prio3_prep_finish_dev")
        return ok

    def aggregate(self, agg_share, out_shares, mask=None):
        n = out_shares.shape[0]
        nat.check(self.L.circl_hip_prio3_aggregate_dev(*self.task, _chk(out_shares, 8), None if mask is None else _chk(mask), _chk(agg_share, 8), n, *self._ws(n),
                                                       _stream()), "prio3_aggregate_dev")
        return agg_share
