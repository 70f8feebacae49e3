"""CPU-side checks of the Prio3 entry points of the C ABI: the argument contract, which is checked before any device is looked for (so
a breach is CIRCL_HIP_EPARAM with or without a GPU), the size queries, Unshard (host only) against the reference's vectors and, without
a GPU, the loud failure of every well-formed call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prio3
from circl_amd import _native as nat
from circl_amd import build as cbuild
from test_oracle_prio3 import FILES, GOLDEN, task_of

KEEP = np.zeros(1 << 16, np.uint64)
P = KEEP.ctypes.data_as(C.c_void_p)
CTX = b"some application"

ENTRY = {   # name -> (its arguments between the task and n, whether its _dev form takes a workspace)
    "shard": (["measurement", "rand", "leader_share", "ok"], True),
    "prep_init": (["agg_id", "verify_key", "nonce", "input_share", "prep_share", "out_share", "ok"], True),
    "prep_finish": (["prep_shares", "ok"], False),
    "aggregate": (["out_share", "mask", "agg_share"], True),
}
OPTIONAL = {"shard": ["ok"], "prep_init": ["ok"], "prep_finish": [], "aggregate": ["mask"]}
FORMS = [(e, s) for e in ENTRY for s in ("", "_dev")]
TYPES = [(1, 0), (2, 1), (2, 255), (2, 2**63 - 1)]


@pytest.fixture(scope="module")
def L():
    cbuild.build()
    return nat.lib()


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def call(lib, entry, suffix, n=1, kind=2, mx=255, shares=2, ctx=CTX, ctx_len=None, ws=P, ws_bytes=None, **over):
    """the entry point with well-formed arguments, except for what is given"""
    names, has_ws = ENTRY[entry]
    args = [over.get(a, 0 if a == "agg_id" else P) for a in names]
    tail = [n]
    if suffix:
        if has_ws:
            tail += [ws, lib.circl_hip_prio3_workspace_size(kind, mx % 2**64, n) if ws_bytes is None else ws_bytes]
        tail.append(None)
    else:
        tail.append(0)
    return getattr(lib, "circl_hip_prio3_" + entry + suffix)(kind, mx, shares, ctx, len(ctx) if ctx_len is None else ctx_len, *args, *tail)


def test_the_constants_and_the_kernel_ids():
    with open(os.path.join(cbuild.ROOT, "include", "circl_hip.h")) as f:
        d = dict(re.findall(r"#define (CIRCL_HIP_\w+) (\d+)", f.read()))
    assert (d["CIRCL_HIP_PRIO3_COUNT"], d["CIRCL_HIP_PRIO3_SUM"], d["CIRCL_HIP_KERNEL_COUNT"]) == ("1", "2", "46")


def test_size_queries(L):
    assert L.circl_hip_prio3_leader_share_size(1, 0) == 48 and L.circl_hip_prio3_prep_share_size(1) == 32
    assert L.circl_hip_prio3_prep_share_size(2) == 24
    for b, p in [(1, 4), (2, 8), (3, 8), (4, 16), (7, 16), (8, 32), (15, 32), (16, 64), (31, 64), (32, 128), (63, 128)]:
        for mx in {2**b - 1, 2**(b - 1)}:
            assert L.circl_hip_prio3_leader_share_size(2, mx) == 8 * (2 * b + 2 * p) == prio3.Task(2, mx, 2, b"").leader_share_size, (b, mx)
            for n in (1, 64, 65, 4096):
                assert L.circl_hip_prio3_workspace_size(2, mx, n) == max(8192, -(-8 * (2 * p + 2 * b + 1) * (-(-n // 64) * 64) // 256) * 256)
    for shares in (2, 3, 255):
        assert L.circl_hip_prio3_rand_size(shares) == 32 * shares
    for shares in (-1, 0, 1, 256, 1000):
        assert L.circl_hip_prio3_rand_size(shares) == 0
    for kind, mx in [(0, 0), (3, 0), (1, 1), (2, 0), (2, 2**63), (2, 2**64 - 1), (-1, 0)]:
        assert L.circl_hip_prio3_leader_share_size(kind, mx) == 0 and L.circl_hip_prio3_workspace_size(kind, mx, 64) == 0
    for kind in (0, 3, -1):
        assert L.circl_hip_prio3_prep_share_size(kind) == 0
    assert L.circl_hip_prio3_workspace_size(1, 0, 1) == 8192 and L.circl_hip_prio3_workspace_size(1, 0, 1 << 20) == 8 * 10 << 20


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_a_well_formed_call_passes_the_contract(L, entry, suffix):
    for kind, mx in TYPES:
        for shares in (2, 3, 255):
            for ctx in (b"", CTX, bytes(255)):
                kw = dict(kind=kind, mx=mx, shares=shares, ctx=ctx)
                assert call(L, entry, suffix, n=0, **kw) == nat.OK
                if _no_gpu():   # (with a GPU these host pointers must not reach a kernel)
                    assert call(L, entry, suffix, **kw) == nat.ENODEV
    assert call(L, entry, suffix, n=0, ctx=None, ctx_len=0) == nat.OK
    if _no_gpu():
        for k in OPTIONAL[entry]:
            assert call(L, entry, suffix, **{k: None}) == nat.ENODEV
        if entry == "prep_init":
            assert call(L, entry, suffix, shares=3, agg_id=2) == nat.ENODEV


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_the_bounds_of_a_task(L, entry, suffix):
    for n in (0, 1):
        for kind, mx in [(0, 0), (3, 0), (-1, 0), (1, 1), (1, 255), (2, 0), (2, 2**63), (2, 2**64 - 1)]:
            assert call(L, entry, suffix, n, kind=kind, mx=mx) == nat.EPARAM, (kind, mx)
        for shares in (-1, 0, 1, 256, 257):
            assert call(L, entry, suffix, n, shares=shares) == nat.EPARAM, shares
        assert call(L, entry, suffix, n, ctx=bytes(256)) == nat.EPARAM
        assert call(L, entry, suffix, n, ctx=None, ctx_len=3) == nat.EPARAM
        if entry == "prep_init":
            for shares, agg_id in [(2, 2), (2, -1), (3, 3), (255, 255), (2, 256)]:
                assert call(L, entry, suffix, n, shares=shares, agg_id=agg_id) == nat.EPARAM, (shares, agg_id)


@pytest.mark.parametrize("entry,suffix", FORMS)
def test_required_pointers(L, entry, suffix):
    for k in ENTRY[entry][0]:
        if k == "agg_id" or k in OPTIONAL[entry]:
            continue
        assert call(L, entry, suffix, **{k: None}) == nat.EPARAM, k
        assert call(L, entry, suffix, 0, **{k: None}) == nat.OK


def test_misaligned_device_pointers_and_small_workspaces(L):
    odd = C.c_void_p(KEEP.ctypes.data + 4)
    for entry, (names, has_ws) in ENTRY.items():
        for k in names:
            if k in ("agg_id", "ok", "mask"):
                continue
            assert call(L, entry, "_dev", **{k: odd}) == nat.EWORKSPACE, (entry, k)
            assert call(L, entry, "_dev", kind=3, **{k: odd}) == nat.EPARAM      # the contract comes first
        if has_ws:
            assert call(L, entry, "_dev", ws=odd) == nat.EWORKSPACE
            assert call(L, entry, "_dev", ws=None) == nat.EWORKSPACE
            assert call(L, entry, "_dev", n=65, ws_bytes=L.circl_hip_prio3_workspace_size(2, 255, 64) - 1 if entry != "aggregate" else 8191) == nat.EWORKSPACE
            assert call(L, entry, "_dev", n=0, ws=None, ws_bytes=0) == nat.OK


def _unshard(L, t, agg, num):
    a, res = np.frombuffer(b"".join(agg), np.uint8).copy(), C.c_uint64(0)
    rc = L.circl_hip_prio3_unshard(t.kind, t.max, t.shares, t.ctx, len(t.ctx), a.ctypes.data_as(C.c_void_p), num, C.byref(res))
    return rc, res.value


@pytest.mark.parametrize("name", FILES)
def test_unshard_on_the_vectors(L, name):
    v = GOLDEN["files"][name]
    assert _unshard(L, task_of(v), [bytes.fromhex(a) for a in v["agg_shares"]], len(v["prep"])) == (nat.OK, v["agg_result"])


def test_unshard_bounds(L):
    t = prio3.Task(2, 2**62, 2, b"")
    agg = [(5).to_bytes(8, "little"), (prio3.P - 2).to_bytes(8, "little")]
    assert _unshard(L, t, agg, 3) == (nat.OK, 3)
    assert _unshard(L, t, agg, 4)[0] == nat.EPARAM                                # 2^64 > p - 1
    assert _unshard(L, t, agg, 2**40)[0] == nat.EPARAM
    small = prio3.Task(2, 3, 2, b"")
    assert _unshard(L, small, agg, (prio3.P - 1) // 3) == (nat.OK, 3)
    assert _unshard(L, small, agg, (prio3.P - 1) // 3 + 1)[0] == nat.EPARAM
    assert _unshard(L, prio3.Task(1, 0, 2, b""), agg, 2**64 - 1) == (nat.OK, 3)   # Count has no bound
    assert _unshard(L, small, [agg[0], prio3.P.to_bytes(8, "little")], 1)[0] == nat.EPARAM   # not canonical
    assert L.circl_hip_prio3_unshard(2, 3, 2, b"", 0, None, 1, C.byref(C.c_uint64())) == nat.EPARAM
    assert L.circl_hip_prio3_unshard(2, 0, 2, b"", 0, P, 1, C.byref(C.c_uint64())) == nat.EPARAM


def test_no_gpu_means_loud_failure(L):
    from circl_amd import hostapi as api
    for kind, mx in TYPES:
        c = api.Prio3(kind, mx, 3, CTX)
        t = prio3.Task(kind, mx, 3, CTX)
        assert (c.leader_share_size, c.prep_share_size, c.rand_size) == (t.leader_share_size, t.prep_share_size, 96)
        if _no_gpu():
            for f in (lambda: c.shard([0, 1], np.zeros((2, 96), np.uint8)), lambda: c.prep_init(1, bytes(32), np.zeros((2, 16), np.uint8), np.zeros((2, 32), np.uint8)),
                      lambda: c.prep_finish(np.zeros((2, 3 * c.prep_share_size), np.uint8)), lambda: c.aggregate(bytes(8), np.zeros((2, 8), np.uint8))):
                with pytest.raises(nat.CirclHipError) as e:
                    f()
                assert e.value.code == nat.ENODEV
        assert c.unshard([bytes(8)] * 3, 1) == 0
        with pytest.raises(ValueError):
            c.shard([0, 1], np.zeros((3, 96), np.uint8))
    for bad in ((0, 0, 2, b""), (1, 1, 2, b""), (2, 0, 2, b""), (2, 2**63, 2, b""), (2, 5, 1, b""), (2, 5, 256, b""), (2, 5, 2, bytes(256))):
        with pytest.raises(ValueError):
            api.Prio3(*bad)
