"""Round-2 surface: key tables (grouped keys), the staged host-buffer pipeline (misaligned pageable pointers, chunk
boundaries, concurrent callers), context rules at the ABI boundary, multi-device plumbing on a 1-GPU box, and the bench
harness itself at a small size.  Everything goes through the C ABI; the oracle is the checker."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from benchrec import bench_record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- key tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", [512, 768, 1024])
@pytest.mark.parametrize("nkeys", [1, 7, 1000])
def test_mlkem_keyed_equals_per_item_api(param, nkeys):
    from circl_amd import hostapi
    from oracle import orc
    rng = np.random.default_rng(param + nkeys)
    n = 3001
    ek, dk = orc.mlkem_keygen(param, rng.integers(0, 256, (nkeys, 64), dtype=np.uint8))
    if nkeys > 2:
        ek[2, 0:2] = 0xFF  # a non-canonical table entry: its items get status 1
        dk[1, -40] ^= 1    # a private key whose stored hash does not match: status 2
    idx = rng.integers(0, nkeys, n).astype(np.uint32)
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ct, ss, st = hostapi.mlkem_encaps_keyed(param, ek, idx, m)
    ct0, ss0, st0 = hostapi.mlkem_encaps(param, ek[idx], m)
    assert (st == st0).all() and (ct == ct0).all() and (ss == ss0).all()
    cto, sso, sto = orc.mlkem_encaps(param, ek[idx[:256]], m[:256])
    assert (st[:256] == sto).all() and (ct[:256] == cto).all() and (ss[:256] == sso).all()
    if nkeys > 2:
        assert st[idx == 2].all() and not st[idx != 2].any()
    # decapsulation with the key table (ciphertexts of the canonical keys; some corrupted -> implicit rejection)
    ct_in = ct.copy()
    ct_in[::5, 10] ^= 0x40
    ss2, st2 = hostapi.mlkem_decaps_keyed(param, dk, idx, ct_in)
    ss20, st20 = hostapi.mlkem_decaps(param, dk[idx], ct_in)
    assert (st2 == st20).all() and (ss2 == ss20).all()
    sso2, sto2 = orc.mlkem_decaps(param, dk[idx[:256]], ct_in[:256])
    assert (st2[:256] == sto2).all() and (ss2[:256] == sso2).all()
    if nkeys > 2:
        assert (st2[idx == 1] == 2).all()


def test_mlkem_keyed_bad_index_is_refused():
    from circl_amd import _native as nat
    from circl_amd import hostapi
    ek = np.zeros((3, 1184), np.uint8)
    with pytest.raises(nat.CirclHipError):
        hostapi.mlkem_encaps_keyed(768, ek, np.array([0, 3], np.uint32), np.zeros((2, 32), np.uint8))


@pytest.mark.parametrize("param", [44, 65, 87, 3])
@pytest.mark.parametrize("nkeys", [1, 7, 300])
def test_mldsa_verify_keyed_equals_per_item_api(param, nkeys):
    from circl_amd import hostapi
    from oracle import orc
    rng = np.random.default_rng(100 * param + nkeys)
    n = 1200
    pk, sk = hostapi.mldsa_keygen(param, rng.integers(0, 256, (nkeys, 32), dtype=np.uint8))
    idx = rng.integers(0, nkeys, n).astype(np.uint32)
    msgs = [rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes() for _ in range(n)]
    ctxs = None if param == 3 else [rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes() for _ in range(n)]
    sig = hostapi.mldsa_sign(param, sk[idx], msgs, ctxs)
    bad = rng.choice(n, n // 10, replace=False)
    sig[bad, 40 + (bad % 1000)] ^= 2
    ok = hostapi.mldsa_verify_keyed(param, pk, idx, sig, msgs, ctxs)
    ok0 = hostapi.mldsa_verify(param, pk[idx], sig, msgs, ctxs)
    assert (ok == ok0).all()
    want = np.ones(n, np.uint8)
    want[bad] = 0
    assert (ok == want).all()
    oko = orc.mldsa_verify(param, pk[idx[:200]], sig[:200], msgs[:200], None if ctxs is None else ctxs[:200])
    assert (ok[:200] == oko).all()


def test_keyed_device_resident_matches_and_is_fast_enough():
    # throughput criterion of the key-table API: within 10 % of the shared-key rate for k <= 1000 (measured, printed)
    import torch
    from circl_amd import device as cdev
    n, nkeys = 1 << 18, 1000
    g = torch.Generator(device="cuda").manual_seed(5)
    seeds = torch.randint(0, 256, (nkeys, 64), dtype=torch.uint8, device="cuda", generator=g)
    m = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    idx = torch.randint(0, nkeys, (n,), dtype=torch.int32, device="cuda", generator=g)
    ek, dk = cdev.MLKEMDevice(768, nkeys).keygen(seeds)
    eng = cdev.MLKEMDevice(768, n)
    ct_k, ss_k, st_k = (torch.empty_like(eng.ct), torch.empty_like(eng.ss), torch.empty_like(eng.status))
    eng.encaps_keyed(ek, idx, m, ct_k, ss_k, st_k)
    eng.encaps(ek[idx.long()].contiguous(), m)
    torch.cuda.synchronize()
    assert bool((ct_k == eng.ct).all()) and bool((ss_k == eng.ss).all()) and int(st_k.sum()) == 0

    def timeit(fn):
        fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / 5
    t_keyed = timeit(lambda: eng.encaps_keyed(ek, idx, m, ct_k, ss_k, st_k))
    t_shared = timeit(lambda: eng.encaps_shared(ek[:1], m, ct_k, ss_k, st_k))
    print(f"ML-KEM-768 n=2^18: keyed(1000 keys) {n / t_keyed * 1e3:.3e}/s  shared {n / t_shared * 1e3:.3e}/s")
    assert t_keyed < 1.25 * t_shared
    # decapsulation through the table round-trips
    ss_d, st_d = torch.empty_like(eng.ss), torch.empty_like(eng.status)
    eng.decaps_keyed(dk, idx, eng.ct, ss_d, st_d)
    torch.cuda.synchronize()
    assert bool((ss_d == eng.ss).all()) and int(st_d.sum()) == 0


# ---- host-buffer pipeline ---------------------------------------------------------------------------------------
def test_host_api_accepts_misaligned_pageable_pointers():
    # a Go sub-slice is 1-byte aligned: every host array deliberately sits at an odd offset
    from circl_amd import _native as nat
    from oracle import orc
    L = nat.lib()
    rng = np.random.default_rng(77)
    n = 5000
    ek, dk = orc.mlkem_keygen(768, rng.integers(0, 256, (n, 64), dtype=np.uint8))
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def odd(a, off):
        raw = np.zeros(a.size + 64, np.uint8)
        v = raw[off:off + a.size]
        v[:] = a.reshape(-1)
        return v
    g_ek, g_m = odd(ek, 1), odd(m, 3)
    g_ct, g_ss, g_st = odd(np.zeros(n * 1088, np.uint8), 5), odd(np.zeros(n * 32, np.uint8), 7), odd(np.zeros(n, np.uint8), 9)
    assert L.circl_hip_mlkem_encaps(768, _p(g_ek), _p(g_m), _p(g_ct), _p(g_ss), _p(g_st), n, 0) == 0
    ct0, ss0, _ = orc.mlkem_encaps(768, ek, m)
    assert (g_ct.reshape(n, 1088) == ct0).all() and (g_ss.reshape(n, 32) == ss0).all() and not g_st.any()
    g_dk = odd(dk, 11)
    g_ss2, g_st2 = odd(np.zeros(n * 32, np.uint8), 13), odd(np.zeros(n, np.uint8), 15)
    assert L.circl_hip_mlkem_decaps(768, _p(g_dk), _p(g_ct), _p(g_ss2), _p(g_st2), n, 0) == 0
    assert (g_ss2 == g_ss).all() and not g_st2.any()
    # status == NULL and n == 0 as cgo would pass them
    assert L.circl_hip_mlkem_encaps(768, _p(g_ek), _p(g_m), _p(g_ct), _p(g_ss), None, n, 0) == 0
    assert L.circl_hip_mlkem_encaps(768, None, None, None, None, None, 0, 0) == 0


def test_host_api_pinned_and_pageable_agree():
    from circl_amd import _native as nat
    from oracle import orc
    L = nat.lib()
    rng = np.random.default_rng(78)
    n = 4096
    ek, _ = orc.mlkem_keygen(768, rng.integers(0, 256, (n, 64), dtype=np.uint8))
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ct_p = np.zeros((n, 1088), np.uint8); ss_p = np.zeros((n, 32), np.uint8); st_p = np.zeros(n, np.uint8)
    assert L.circl_hip_mlkem_encaps(768, _p(ek), _p(m), _p(ct_p), _p(ss_p), _p(st_p), n, 0) == 0

    def pinned(a):
        p = L.circl_hip_alloc_host(a.size)
        v = np.ctypeslib.as_array((C.c_uint8 * a.size).from_address(p))
        v[:] = a.reshape(-1)
        return p, v
    p_ek, _ = pinned(ek); p_m, _ = pinned(m)
    p_ct, v_ct = pinned(np.zeros(n * 1088, np.uint8)); p_ss, v_ss = pinned(np.zeros(n * 32, np.uint8)); p_st, v_st = pinned(np.zeros(n, np.uint8))
    assert L.circl_hip_mlkem_encaps(768, p_ek, p_m, p_ct, p_ss, p_st, n, 0) == 0
    assert (v_ct.reshape(n, 1088) == ct_p).all() and (v_ss.reshape(n, 32) == ss_p).all()
    for p in (p_ek, p_m, p_ct, p_ss, p_st):
        L.circl_hip_free_host(p)


def test_host_api_three_concurrent_callers():
    # entry points are re-entrant: three host threads call the host-buffer API at once (different operations)
    from circl_amd import hostapi
    from oracle import orc
    rng = np.random.default_rng(79)
    n = 20000
    ek, dk = orc.mlkem_keygen(768, rng.integers(0, 256, (n, 64), dtype=np.uint8))
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ct0, ss0, _ = orc.mlkem_encaps(768, ek, m)
    pk, sk = orc.mldsa_keygen(65, rng.integers(0, 256, (64, 32), dtype=np.uint8))
    msgs = [bytes([i]) * 40 for i in range(64)]
    sig = orc.mldsa_sign(65, sk, msgs)
    res, errs = {}, []

    def enc():
        try:
            for _ in range(3):
                res["enc"] = hostapi.mlkem_encaps(768, ek, m)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def dec():
        try:
            for _ in range(3):
                res["dec"] = hostapi.mlkem_decaps(768, dk, ct0)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def ver():
        try:
            for _ in range(6):
                res["ver"] = hostapi.mldsa_verify(65, pk, sig, msgs)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=f) for f in (enc, dec, ver)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert (res["enc"][0] == ct0).all() and (res["enc"][1] == ss0).all()
    assert (res["dec"][0] == ss0).all() and not res["dec"][1].any()
    assert res["ver"].all()


def _run_py(code, env_extra=None, timeout=240):
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


CHUNK_CODE = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from circl_amd import hostapi
from oracle import orc
rng = np.random.default_rng(5)
n = 3333          # 4 chunks of 2^10 items, the last one ragged; depth-3 pipeline wraps around
ek, dk = orc.mlkem_keygen(768, rng.integers(0, 256, (n, 64), dtype=np.uint8))
m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
ct, ss, st = hostapi.mlkem_encaps(768, ek, m)
ct0, ss0, _ = orc.mlkem_encaps(768, ek, m)
assert (ct == ct0).all() and (ss == ss0).all() and not st.any()
ss2, st2 = hostapi.mlkem_decaps(768, dk, ct)
assert (ss2 == ss0).all() and not st2.any()
# ragged blobs across chunk boundaries: ML-DSA with variable-length messages and contexts
nd = 2500
pk, sk = hostapi.mldsa_keygen(44, rng.integers(0, 256, (nd, 32), dtype=np.uint8))
msgs = [rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for _ in range(nd)]
ctxs = [rng.integers(0, 256, int(rng.integers(0, 50)), dtype=np.uint8).tobytes() for _ in range(nd)]
sig = hostapi.mldsa_sign(44, sk, msgs, ctxs)
assert (sig[:300] == orc.mldsa_sign(44, sk[:300], msgs[:300], ctxs[:300])).all()
sig[7::11, 50] ^= 1
ok = hostapi.mldsa_verify(44, pk, sig, msgs, ctxs)
want = np.ones(nd, np.uint8); want[7::11] = 0
assert (ok == want).all()
# in-place primitive over several chunks
st8 = rng.integers(0, 2**63, (5000, 25), dtype=np.uint64)
out = hostapi.keccak_f1600(st8)
assert (out[:50] == np.stack([orc.keccak_f1600(s) for s in st8[:50]])).all() and (out[-1] == orc.keccak_f1600(st8[-1])).all()
print("chunked ok")
"""


def test_pipeline_chunk_boundaries_small_chunks():
    out = _run_py(CHUNK_CODE % ROOT, {"CIRCL_HIP_HOST_CHUNK": "10"})
    assert "chunked ok" in out


def test_pipeline_single_slot_and_no_worker_threads():
    # degenerate pool sizes must still be correct: one staging slot, zero worker threads (the caller moves the bytes)
    out = _run_py(CHUNK_CODE % ROOT, {"CIRCL_HIP_HOST_CHUNK": "10", "CIRCL_HIP_HOST_SLOTS": "1", "CIRCL_HIP_HOST_THREADS": "0"})
    assert "chunked ok" in out


# ---- context rules at the ABI boundary (mldsa65/dilithium.go:63-65, :116-118; round 3: ErrContextNotSupported) ----
def test_context_rules_host_and_device():
    import torch
    from circl_amd import _native as nat
    from circl_amd import hostapi
    from oracle import orc
    L = nat.lib()
    rng = np.random.default_rng(9)
    n = 40
    pk, sk = orc.mldsa_keygen(65, rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msgs = [b"m%d" % i for i in range(n)]
    long_ctx = [b"" for _ in range(n)]
    long_ctx[3] = bytes(256)
    with pytest.raises(nat.CirclHipError) as e:
        hostapi.mldsa_sign(65, sk, msgs, long_ctx)
    assert e.value.code == nat.EPARAM
    # verify: a too-long context never verifies (no error: sign.Scheme.Verify returns false)
    sig = hostapi.mldsa_sign(65, sk, msgs)
    ok = hostapi.mldsa_verify(65, pk, sig, msgs, long_ctx)
    want = np.ones(n, np.uint8); want[3] = 0
    assert (ok == want).all()
    # round 3: any non-empty context is refused by the host entry points
    pk3, sk3 = orc.mldsa_keygen(3, rng.integers(0, 256, (n, 32), dtype=np.uint8))
    ctx3 = [b"" for _ in range(n)]
    ctx3[5] = b"x"
    with pytest.raises(nat.CirclHipError):
        hostapi.mldsa_sign(3, sk3, msgs, ctx3)
    sig3 = hostapi.mldsa_sign(3, sk3, msgs)
    with pytest.raises(nat.CirclHipError):
        hostapi.mldsa_verify(3, pk3, sig3, msgs, ctx3)
    assert hostapi.mldsa_verify(3, pk3, sig3, msgs, [b""] * n).all()
    # device-resident: the refused item gets an all-zero signature / ok = 0, the others are untouched
    for param, skx, pkx, ctxs, bad in ((65, sk, pk, long_ctx, 3), (3, sk3, pk3, ctx3, 5)):
        PK, SK, SIG = orc.DSA_SIZES[param]
        mb, mo = hostapi._blob(msgs)
        cb, co = hostapi._blob(ctxs)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d_sk, d_mb, d_cb = d(skx), d(mb), d(cb)
        d_mo, d_co = d(mo.astype(np.int64)), d(co.astype(np.int64))
        d_rnd = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_sig = torch.full((n * SIG + 16,), 0xAA, dtype=torch.uint8, device="cuda")
        wsb = L.circl_hip_mldsa_sign_workspace_size(param, n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.circl_hip_mldsa_sign_dev(param, d_sk.data_ptr(), d_mb.data_ptr(), d_mo.data_ptr(), d_cb.data_ptr(), d_co.data_ptr(), d_rnd.data_ptr(), 0,
                                        d_sig.data_ptr(), n, ws.data_ptr(), wsb, st)
        assert rc == 0
        torch.cuda.synchronize()
        got = d_sig[:n * SIG].view(n, SIG).cpu().numpy()
        assert not got[bad].any()
        good = [i for i in range(n) if i != bad]
        ref = orc.mldsa_sign(param, skx[good], [msgs[i] for i in good])
        assert (got[good] == ref).all()
        assert not ws[:128 * n].any().item()  # mu, rho'': the secret part of the workspace is wiped
        d_ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        vwsb = L.circl_hip_mldsa_workspace_size(param, n)
        vws = torch.empty(vwsb, dtype=torch.uint8, device="cuda")
        d_pk = d(pkx)
        rc = L.circl_hip_mldsa_verify_dev(param, d_pk.data_ptr(), d_sig.data_ptr(), d_mb.data_ptr(), d_mo.data_ptr(), d_cb.data_ptr(), d_co.data_ptr(),
                                          d_ok.data_ptr(), n, vws.data_ptr(), vwsb, st)
        assert rc == 0
        torch.cuda.synchronize()
        okv = d_ok.cpu().numpy()
        assert okv[bad] == 0 and okv[good].all()


# ---- multi-device plumbing on a 1-GPU box ---------------------------------------------------------------------
def test_all_devices_equals_device0_and_device_info():
    from circl_amd import _native as nat
    from circl_amd import hostapi
    from oracle import orc
    L = nat.lib()
    nd = L.circl_hip_device_count()
    assert nd >= 1
    cus, numa = C.c_int(0), C.c_int(-2)
    assert L.circl_hip_device_info(0, C.byref(cus), C.byref(numa)) == 0 and cus.value >= 64 and numa.value >= -1
    assert L.circl_hip_device_info(nd, None, None) == nat.ENODEV
    rng = np.random.default_rng(31)
    n = 2001
    ek, dk = orc.mlkem_keygen(768, rng.integers(0, 256, (n, 64), dtype=np.uint8))
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a = hostapi.mlkem_encaps(768, ek, m, device=0)
    b = hostapi.mlkem_encaps(768, ek, m, device=nat.ALL_DEVICES)
    assert all((x == y).all() for x, y in zip(a, b))
    with pytest.raises(nat.CirclHipError):
        hostapi.mlkem_encaps(768, ek, m, device=nd)


def test_two_processes_share_one_visible_device():
    # bench.py --gpus 2 on a 1-GPU box cannot run; what can be checked is that two PROCESSES, each seeing the one GPU
    # as its device 0 through HIP_VISIBLE_DEVICES, run the all-devices path concurrently and agree bit for bit
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from circl_amd import hostapi, _native as nat
from oracle import orc
assert nat.lib().circl_hip_device_count() == 1
rng = np.random.default_rng(11)
n = 6000
ek, dk = orc.mlkem_keygen(1024, rng.integers(0, 256, (n, 64), dtype=np.uint8))
m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
ct, ss, st = hostapi.mlkem_encaps(1024, ek, m, device=nat.ALL_DEVICES)
ct0, ss0, _ = orc.mlkem_encaps(1024, ek, m)
assert (ct == ct0).all() and (ss == ss0).all()
print("proc ok")
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    ps = [subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(2)]
    outs = [p.communicate(timeout=240) for p in ps]
    assert all(p.returncode == 0 for p in ps), outs
    assert all("proc ok" in o[0] for o in outs)


# ---- the bench harness -------------------------------------------------------------------------------------------
def test_bench_py_small_run_emits_every_config(tmp_path):
    xf = str(tmp_path / "extras.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", str(1 << 14), "--no-pmc",
                        "--no-cpu-baseline", "--full", "--extras", "all", "--extras-file", xf], cwd=ROOT, capture_output=True, text=True, timeout=900)
    line, out = bench_record(r, xf)
    assert line["parity"]["bit_exact_vs_oracle"] and line["parity"]["whole_batch"] and line["roofline"]["frac"] > 0
    for k in ("decaps", "config3", "config4", "config5"):
        assert line["configs"][k]["value"] > 0, k
    assert out["metric"].startswith("ML-KEM-768 encapsulations/sec") and out["steps"] == 3 and out["n_gpus"] == 1
    assert out["parity"]["bit_exact_vs_oracle"] and out["parity"]["ranks_failing"] == 0
    # one key per item, and the WHOLE batch went through the oracle (headline and config 4)
    assert out["config"]["key_pool"] == 1 << 14 and out["parity"]["whole_batch"] and out["parity"]["sampled_items"] == 1 << 14
    cfg = out["configs"]
    assert cfg["config4"]["parity"]["whole_batch"]
    # the many-concurrent-callers leg (tools/bin/concurrent_bench, built by build()): coalesced beats uncoalesced, nothing mismatches
    cc = cfg.get("concurrent_callers")
    assert cc and cc["encaps_coalesced"]["T64"]["mismatches"] == 0 and cc["encaps_coalesced"]["T64"]["ops_per_s"] > 2 * cc["encaps_uncoalesced"]["T64"]["ops_per_s"]
    ar = cc["async_reactors"]  # the submit / poll form: R reactors x W outstanding one-item requests, every result compared by the tool
    assert all(v.get("mismatches") == 0 and v["items_per_s"] > 0 for v in ar.values()), ar
    assert ar["encaps_R4_W128"]["items_per_s"] > cc["encaps_coalesced"]["T64"]["ops_per_s"]
    assert out["roofline"]["valu"] is None or out["roofline"]["valu"]["ceiling_source"] in ("live", None)  # (--no-pmc: no instruction count to price)
    for k in ("decaps", "config3", "config4", "config5", "host_abi", "shared_key", "keyed"):
        assert k in cfg, k
    assert cfg["decaps"]["parity"]["bit_exact_vs_oracle"] and cfg["decaps"]["parity"]["all_items_ss_dec_equals_ss_enc"]
    assert cfg["config4"]["parity"]["bit_exact_vs_oracle"] and cfg["config4"]["parity"]["all_items_as_expected"]
    assert cfg["config4"]["parity"]["gpu_signatures_equal_oracle"]["bit_exact_vs_oracle"]
    assert cfg["config5"]["parity"]["ranks_failing"] == 0
    assert cfg["host_abi"]["pageable"]["all_ct_equal_device_resident_run"] and cfg["host_abi"]["pinned"]["all_ct_equal_device_resident_run"]
    assert cfg["keyed"]["equals_per_item_api_on_gathered_keys"]
    assert out["roofline"]["frac"] > 0


@pytest.mark.parametrize("mode", ["encaps", "host"])
def test_bench_py_plain_run_times_its_steps_and_dumps_its_outputs(mode, tmp_path):
    # a plain run (no --full) is the headline alone: exactly --steps timed steps, no parity / roofline / CPU baseline / record file;
    # --dump-outputs holds what the last timed step computed (every row at this size), equal to the oracle's on the same seeded inputs
    import bench
    from oracle import orc
    B, d, xf = 1 << 12, tmp_path / "out", tmp_path / "extras.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--batch", str(B), "--mode", mode,
                        "--dump-outputs", str(d), "--extras-file", str(xf)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["config"]["mode"] == mode and line["ms_per_step"] > 0 and line["higher_is_better"]
    assert abs(line["value"] - B * 1e3 / line["ms_per_step"]) <= 1e-4 * line["value"]
    assert all(line.get(k) is None for k in ("parity", "roofline", "cpu_baseline", "strong", "configs", "value_host_abi")), line
    assert not xf.exists()
    rows = np.load(d / "sample_rows.npy")
    assert rows.dtype == np.float64 and (rows == np.arange(B)).all()
    ct, ss, st = (np.load(d / (n + ".npy")) for n in ("ciphertext", "shared_secret", "status"))
    assert ct.dtype == ss.dtype == st.dtype == np.float32 and ct.shape == (B, 1088) and ss.shape == (B, 32) and st.shape == (B,)
    ek, _dk = orc.mlkem_keygen(768, bench.shake_seeds("circl-hip/keygen", B, 64))
    ct0, ss0, st0 = orc.mlkem_encaps(768, ek, bench.shake_seeds("circl-hip/m", B, 32))
    assert (ct == ct0).all() and (ss == ss0).all() and not st.any() and not st0.any()


def test_bench_py_two_ranks_control_flow(tmp_path):
    # bench.py --gpus 2 as the driver launches it (torch.distributed.run, one rank per GPU) cannot run on a 1-GPU box with
    # RCCL; with the process group on gloo and both ranks sharing the one device, everything else of the N > 1 path runs:
    # per-rank batches, barriers, max-over-ranks timing, whole-job aggregation, per-rank gathers, rank 0's JSON line
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, CIRCL_DIST_BACKEND="gloo", CIRCL_BENCH_SHARE_GPU="1")
    xf = str(tmp_path / "extras.json")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", str(1 << 13),
                        "--full", "--extras-file", xf], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    line, out = bench_record(r, xf)
    assert len(line["per_rank"]["encaps_per_s"]) == 2 and line["strong"]["items_per_rank"] == [1 << 12] * 2 and "cpu_baseline" not in line
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["parity"]["ranks_failing"] == 0
    assert len(out["per_rank"]["encaps_per_s"]) == 2
    cfg = out["configs"]
    assert len(cfg["config4"]["per_rank_per_s"]) == 2 and cfg["config4"]["parity"]["ranks_failing"] == 0
    assert len(cfg["config5"]["per_rank_per_s"]) == 2 and cfg["config5"]["parity"]["ranks_failing"] == 0
    assert cfg["decaps"]["parity"]["ranks_failing"] == 0 and len(cfg["host_abi"]["per_rank_pageable_per_s"]) == 2
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only
    # the whole-job value is the sum of the ranks' items over the slowest rank's time
    assert out["value"] <= sum(out["per_rank"]["encaps_per_s"]) * 1.001
