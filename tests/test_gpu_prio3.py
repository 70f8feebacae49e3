"""Prio3Count / Prio3Sum on the GPU (circl_hip_prio3_*), both forms: the reference's vectors in one call per file and operation, the edge
shapes of the kernels (batch sizes around a wavefront, every step of P, the share counts on both sides of the reference's inverse
table) against the checker tests/prio3.py, failure masks, the reduction, the wrappers and the host pipeline's routes
(tests/prio3_worker.py).  Every output lies between sentinels."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import prio3
from test_oracle_prio3 import FILES, GOLDEN, task_of

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
FORMS = ["host", "dev"]
vp = C.c_void_p
P = prio3.P


@pytest.fixture(scope="module")
def L():
    from circl_amd import _native as nat
    return nat.lib()


class Buf:
    """one argument of either form: a host array, or its copy on the device; an output has GUARD sentinel bytes on each side"""

    def __init__(self, form, a=None, out=0):
        import torch
        torch.cuda.set_device(0)
        self.out = out
        self.host = np.full(out + 2 * GUARD, FILL, np.uint8) if a is None else np.array(a).view(np.uint8).reshape(-1)
        self.t = torch.from_numpy(self.host).cuda() if form == "dev" else None

    def ptr(self, at=0):
        return vp((self.t.data_ptr() if self.t is not None else self.host.ctypes.data) + at)

    def body(self):
        """the output between its sentinels, which must have survived"""
        got = self.t.cpu().numpy() if self.t is not None else self.host
        assert (got[:GUARD] == FILL).all() and (got[GUARD + self.out:] == FILL).all()
        return got[GUARD:GUARD + self.out]


class Gpu:
    """the entry points for one task in one form"""

    def __init__(self, L, form, t):
        self.L, self.form, self.t = L, form, t
        self.task = (t.kind, t.max, t.shares, t.ctx, len(t.ctx))
        assert L.circl_hip_prio3_leader_share_size(t.kind, t.max) == t.leader_share_size and L.circl_hip_prio3_prep_share_size(t.kind) == t.prep_share_size

    def _call(self, name, args, n, ws=True):
        fn = getattr(self.L, "circl_hip_prio3_%s%s" % (name, "_dev" if self.form == "dev" else ""))
        if self.form == "dev":
            import torch
            tail = [n]
            if ws:
                size = self.L.circl_hip_prio3_workspace_size(self.t.kind, self.t.max, n)
                w = torch.empty(size, dtype=torch.uint8, device="cuda")
                tail += [vp(w.data_ptr()), size]
            rc = fn(*self.task, *args, *tail, None)
            torch.cuda.synchronize()
        else:
            rc = fn(*self.task, *args, n, 0)
        assert rc == 0, (name, rc, self.L.circl_hip_last_error())

    def shard(self, meas, rands):
        n = len(meas)
        m, r = Buf(self.form, np.array(meas, np.uint64)), Buf(self.form, np.frombuffer(b"".join(rands), np.uint8))
        leader, ok = Buf(self.form, out=n * self.t.leader_share_size), Buf(self.form, out=n)
        self._call("shard", [m.ptr(), r.ptr(), leader.ptr(GUARD), ok.ptr(GUARD)], n)
        b, k = leader.body().tobytes(), self.t.leader_share_size
        return [b[i * k:(i + 1) * k] for i in range(n)], [int(x) for x in ok.body()]

    def prep_init(self, agg_id, vk, nonces, shares):
        n = len(nonces)
        v, nn, sh = Buf(self.form, np.frombuffer(vk, np.uint8)), Buf(self.form, np.frombuffer(b"".join(nonces), np.uint8)), Buf(self.form, np.frombuffer(b"".join(shares), np.uint8))
        prep, out, ok = Buf(self.form, out=n * self.t.prep_share_size), Buf(self.form, out=8 * n), Buf(self.form, out=n)
        self._call("prep_init", [agg_id, v.ptr(), nn.ptr(), sh.ptr(), prep.ptr(GUARD), out.ptr(GUARD), ok.ptr(GUARD)], n)
        pb, ob, k = prep.body().tobytes(), out.body().tobytes(), self.t.prep_share_size
        return [pb[i * k:(i + 1) * k] for i in range(n)], [ob[8 * i:8 * i + 8] for i in range(n)], [int(x) for x in ok.body()]

    def prep_finish(self, rows):
        ps, ok = Buf(self.form, np.frombuffer(b"".join(rows), np.uint8)), Buf(self.form, out=len(rows))
        self._call("prep_finish", [ps.ptr(), ok.ptr(GUARD)], len(rows), ws=False)
        return [int(x) for x in ok.body()]

    def aggregate(self, agg, outs, mask=None):
        o = Buf(self.form, np.frombuffer(b"".join(outs), np.uint8) if isinstance(outs, list) else outs)
        m = None if mask is None else Buf(self.form, np.array(mask, np.uint8))
        a = Buf(self.form, out=8)
        head = np.frombuffer(agg, np.uint8)
        if a.t is not None:
            import torch
            a.t[GUARD:GUARD + 8] = torch.from_numpy(head.copy()).cuda()
        else:
            a.host[GUARD:GUARD + 8] = head
        n = o.host.size // 8
        self._call("aggregate", [o.ptr(), None if m is None else m.ptr(), a.ptr(GUARD)], n)
        return a.body().tobytes()

    def unshard(self, aggs, num):
        a, res = np.frombuffer(b"".join(aggs), np.uint8).copy(), C.c_uint64(0)
        rc = self.L.circl_hip_prio3_unshard(*self.task, a.ctypes.data_as(vp), num, C.byref(res))
        assert rc == (-1 if self.t.kind == prio3.SUM and num * self.t.max >= P else 0)      # (the reference's ErrAggregateBound)
        return None if rc else res.value


# ---- the reference's known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FILES)
def test_whole_fixture(L, form, name):
    v = GOLDEN["files"][name]
    t = task_of(v)
    g = Gpu(L, form, t)
    vk = bytes.fromhex(v["verify_key"])
    rands, nonces = [bytes.fromhex(p["rand"]) for p in v["prep"]], [bytes.fromhex(p["nonce"]) for p in v["prep"]]
    n = len(rands)
    leaders, ok = g.shard([p["measurement"] for p in v["prep"]], rands)
    assert ok == [1] * n and [x.hex() for x in leaders] == [p["input_shares"][0] for p in v["prep"]]
    rows, aggs = [b""] * n, []
    for j in range(t.shares):
        prep, out, ok = g.prep_init(j, vk, nonces, leaders if j == 0 else [r[32 * (j - 1):32 * j] for r in rands])
        assert ok == [1] * n
        assert [x.hex() for x in prep] == [p["prep_shares"][0][j] for p in v["prep"]]
        assert [[x.hex()] for x in out] == [p["out_shares"][j] for p in v["prep"]]
        rows = [a + b for a, b in zip(rows, prep)]
        aggs.append(g.aggregate(bytes(8), out))
    assert g.prep_finish(rows) == [1] * n
    assert [a.hex() for a in aggs] == v["agg_shares"] and g.unshard(aggs, n) == v["agg_result"]


# ---- edge shapes against the checker ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(kind, mx, shares, n, agg_ids):
    """the checker's run of n good reports, computed once per shape and shared by both forms"""
    rng = random.Random(kind * 7919 + mx % 1009 + 31 * shares + n)
    t = prio3.Task(kind, mx, shares, b"edge shapes")
    vk = rng.randbytes(32)
    rands, nonces = [rng.randbytes(t.rand_size) for _ in range(n)], [rng.randbytes(16) for _ in range(n)]
    meas = [rng.randrange(mx + 1) if kind == 2 else rng.randrange(2) for _ in range(n)]
    meas[0], meas[-1] = (mx, 0) if kind == 2 else (1, 0)
    leaders = [t.shard(m, r) for m, r in zip(meas, rands)]
    preps = {j: [t.prep_init(j, vk, nonces[i], leaders[i] if j == 0 else rands[i][32 * (j - 1):32 * j]) for i in range(n)] for j in agg_ids}
    return t, vk, rands, nonces, meas, leaders, preps


def flow(L, form, kind, mx, shares, n):
    agg_ids = tuple(range(shares)) if shares <= 3 else (0, 1, shares - 1)
    t, vk, rands, nonces, meas, leaders, preps = expected(kind, mx, shares, n, agg_ids)
    g = Gpu(L, form, t)
    got, ok = g.shard(meas, rands)
    assert ok == [1] * n and got == leaders
    rows, aggs = [b""] * n, []
    for j in agg_ids:
        prep, out, ok = g.prep_init(j, vk, nonces, leaders if j == 0 else [r[32 * (j - 1):32 * j] for r in rands])
        assert ok == [1] * n and list(zip(prep, out)) == preps[j], j
        rows = [a + b for a, b in zip(rows, prep)]
        start = (P - 1 - j).to_bytes(8, "little")
        agg = g.aggregate(start, out)
        assert agg == prio3.aggregate(start, out)
        aggs.append(prio3.aggregate(agg, [(1 + j).to_bytes(8, "little")]))
    if len(agg_ids) == shares:   # the whole flow ends in the right sum
        assert g.prep_finish(rows) == [1] * n
        assert g.unshard(aggs, n) == (None if kind == 2 and n * mx >= P else sum(meas))


TYPES = [(1, 0, 257), (2, 1, 257), (2, 2, 63), (2, 7, 64), (2, 8, 65), (2, 255, 1), (2, 1337, 63), (2, 2**16 - 1, 64), (2, 2**31, 65), (2, 2**63 - 1, 65)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,mx,n", TYPES)
def test_every_step_of_p(L, form, kind, mx, n):
    flow(L, form, kind, mx, 2, n)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shares,n", [(3, 64), (8, 63), (9, 1), (255, 65)])
def test_share_counts(L, form, shares, n):
    flow(L, form, 2, 255, shares, n)
    if shares == 3:
        flow(L, form, 1, 0, shares, 65)


# ---- failure masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,mx", [(1, 0), (2, 1337)])
def test_failure_masks(L, form, kind, mx):
    """a shuffled batch, a third of it bad in every way: a measurement out of range, a leader share and a prep share that are not
    canonical, a flipped proof-share byte, a cheating client"""
    rng = random.Random(kind + mx)
    t = prio3.Task(kind, mx, 2, b"failure masks")
    g = Gpu(L, form, t)
    n = 90
    how = ["good"] * 60 + ["range", "leader", "prep", "flip", "cheat"] * 6
    rng.shuffle(how)
    vk = rng.randbytes(32)
    rands, nonces = [rng.randbytes(t.rand_size) for _ in range(n)], [rng.randbytes(16) for _ in range(n)]
    meas = [rng.randrange(mx + 1) if kind == 2 else rng.randrange(2) for _ in range(n)]
    sent = [(mx + 1 + rng.randrange(3) if kind == 2 else 2 + rng.randrange(3)) if h == "range" else m for m, h in zip(meas, how)]
    leaders, ok = g.shard(sent, rands)
    assert ok == [int(h != "range") for h in how]
    for i, h in enumerate(how):
        assert leaders[i] == (bytes(t.leader_share_size) if h == "range" else t.shard(meas[i], rands[i])), (i, h)
    for i, h in enumerate(how):
        x = leaders[i]
        if h == "leader":
            at = 8 * rng.randrange(t.leader_share_size // 8)
            leaders[i] = x[:at] + (P + rng.randrange(2**32 - 1)).to_bytes(8, "little") + x[at + 8:]
        elif h == "flip":
            at = 8 * t.meas_len + rng.randrange(t.leader_share_size - 8 * t.meas_len - 1)
            leaders[i] = x[:at] + bytes([x[at] ^ 1]) + x[at + 1:]      # (the low seven bytes of an element: it stays canonical)
            if prio3.dec(leaders[i]) is None:
                leaders[i] = x[:at] + bytes([x[at] ^ 2]) + x[at + 1:]
        elif h == "cheat":
            enc = t.encode(meas[i])
            enc[rng.randrange(t.meas_len)] = 2 + rng.randrange(5)
            leaders[i] = t.shard_encoded(enc, rands[i])
        elif h == "range":
            leaders[i] = t.shard(0, rands[i])        # (a good report in its place, so that the later steps have one)
    rows = [b""] * n
    for j in range(2):
        shares_j = leaders if j == 0 else [r[:32] for r in rands]
        prep, out, ok = g.prep_init(j, vk, nonces, shares_j)
        for i, h in enumerate(how):
            if j == 0 and h == "leader":
                assert ok[i] == 0 and prep[i] == bytes(t.prep_share_size) and out[i] == bytes(8), i
            else:
                assert ok[i] == 1 and (prep[i], out[i]) == t.prep_init(j, vk, nonces[i], shares_j[i]), (i, h)
        rows = [a + b for a, b in zip(rows, prep)]
    for i, h in enumerate(how):
        if h == "prep":
            at = 8 * rng.randrange(2 * t.prep_share_size // 8)
            rows[i] = rows[i][:at] + (2**64 - 1 - rng.randrange(2**32 - 1)).to_bytes(8, "little") + rows[i][at + 8:]
    verdict = g.prep_finish(rows)
    assert verdict == [int(t.prep_finish(r)) for r in rows]
    assert verdict == [int(h in ("good", "range")) for h in how]


# ---- the reduction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 64, 65, 4097, 65537])
def test_aggregate(L, form, n):
    rng = np.random.default_rng(n)
    g = Gpu(L, form, prio3.Task(1, 0, 2, b""))
    out = rng.integers(0, P, n, dtype=np.uint64)
    out[0], out[-1] = P - 1, P - 1
    mask = (rng.integers(0, 3, n) != 0).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    start = int(rng.integers(0, P, dtype=np.uint64))
    ints = [int(x) for x in out]
    assert g.aggregate(start.to_bytes(8, "little"), out) == ((start + sum(ints)) % P).to_bytes(8, "little")
    assert g.aggregate((P - 1).to_bytes(8, "little"), out, mask) == ((P - 1 + sum(x for x, m in zip(ints, mask) if m)) % P).to_bytes(8, "little")


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mx", [(1, 0), (2, 1000)])
def test_the_wrappers_agree_with_the_checker(kind, mx):
    import torch
    from circl_amd import device as dev
    from circl_amd import hostapi as api
    n, shares = 70, 3
    t, vk, rands, nonces, meas, leaders, preps = expected(kind, mx, shares, n, (0, 1, 2))
    h, d = api.Prio3(kind, mx, shares, t.ctx), dev.Prio3Device(kind, mx, shares, t.ctx)
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    rand_a, nonce_a = np.frombuffer(b"".join(rands), np.uint8).reshape(n, -1), np.frombuffer(b"".join(nonces), np.uint8).reshape(n, 16)
    lh, okh = h.shard(meas, rand_a)
    ld, okd = d.shard(cu(np.array(meas, np.int64)), cu(rand_a))
    assert okh.all() and okd.cpu().numpy().all()
    assert [r.tobytes() for r in lh] == leaders and (ld.cpu().numpy() == lh).all()
    rows_h, aggs = np.zeros((n, shares, t.prep_share_size), np.uint8), []
    rows_d = torch.zeros((n, shares, t.prep_share_size), dtype=torch.uint8, device="cuda")
    for j in range(shares):
        sh = lh if j == 0 else rand_a[:, 32 * (j - 1):32 * j]
        ph, oh, okh = h.prep_init(j, vk, nonce_a, sh)
        pd, od, okd = d.prep_init(j, cu(np.frombuffer(vk, np.uint8)), cu(nonce_a), ld if j == 0 else cu(sh))
        assert okh.all() and okd.cpu().numpy().all()
        assert [(a.tobytes(), b.tobytes()) for a, b in zip(ph, oh)] == preps[j]
        assert (pd.cpu().numpy() == ph).all() and (od.cpu().numpy() == oh).all()
        rows_h[:, j], rows_d[:, j] = ph, pd
        agg_d = d.aggregate(torch.zeros(8, dtype=torch.uint8, device="cuda"), od)
        aggs.append(h.aggregate(bytes(8), oh))
        assert agg_d.cpu().numpy().tobytes() == aggs[-1]
    assert h.prep_finish(rows_h).all() and d.prep_finish(rows_d.contiguous()).cpu().numpy().all()
    assert h.unshard(aggs, n) == sum(meas)


def test_a_misaligned_device_pointer(L):
    """and a workspace that is too small; nothing is launched"""
    import torch
    from circl_amd import _native as nat
    t = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    need = L.circl_hip_prio3_workspace_size(2, 255, 4)
    assert need == 8 * (2 * 32 + 16 + 1) * 64
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p, odd, task = vp(t.data_ptr()), vp(t.data_ptr() + 4), (2, 255, 2, b"", 0)
    assert L.circl_hip_prio3_shard_dev(*task, p, odd, p, p, 4, vp(ws.data_ptr()), need, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_shard_dev(*task, p, p, p, p, 4, vp(ws.data_ptr() + 4), need - 4, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_shard_dev(*task, p, p, p, p, 4, vp(ws.data_ptr()), need - 1, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_prep_init_dev(*task, 1, p, p, p, p, odd, p, 4, vp(ws.data_ptr()), need, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_prep_finish_dev(*task, odd, p, 4, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_aggregate_dev(*task, p, None, odd, 4, vp(ws.data_ptr()), need, None) == nat.EWORKSPACE
    assert L.circl_hip_prio3_aggregate_dev(*task, p, None, p, 4, vp(ws.data_ptr()), 8191, None) == nat.EWORKSPACE
    torch.cuda.synchronize()
    assert not t.any().item()


# ---- the host pipeline's routes -------------------------------------------------------------------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 items at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices
SPOTS = (0, 7, 99, 100, 199, 200, 255, 256, 299)


@pytest.fixture(scope="module")
def pipe(L):
    """this process's own run with the default settings -- one chunk at lo = 0 -- computed once and shared"""
    import prio3_worker as pw
    return pw.run(L, 0, N_PIPE)


def _check_pipeline_run(o, base):
    """what every configuration asserts about one run of prio3_worker.run"""
    import prio3_worker as pw
    for k in base:
        assert o[k].shape == base[k].shape and (np.asarray(o[k]) == base[k]).all(), k
    for name, kind, mx, shares in pw.TASKS:
        t = prio3.Task(kind, mx, shares, pw.CTX)
        meas, rand, nonce, vk = pw.inputs(name, N_PIPE)
        good = [int(i not in pw.BAD) for i in range(N_PIPE)]
        assert o[name + "_ok"].tolist() == good and o[name + "_verdict"].tolist() == good
        leader = o[name + "_leader"].reshape(N_PIPE, -1)
        preps = o[name + "_preps"].reshape(N_PIPE, shares, -1)
        for i in SPOTS:
            if not good[i]:
                assert not leader[i].any()
                continue
            assert leader[i].tobytes() == t.shard(int(meas[i]), rand[i].tobytes()), (name, i)
            for j in range(shares):
                want = t.prep_init(j, vk.tobytes(), nonce[i].tobytes(), leader[i].tobytes() if j == 0 else rand[i, 32 * (j - 1):32 * j].tobytes())
                assert (preps[i, j].tobytes(), o["%s_out%d" % (name, j)][8 * i:8 * i + 8].tobytes()) == want, (name, i, j)
        aggs = [o["%s_agg%d" % (name, j)].tobytes() for j in range(shares)]
        assert t.unshard(aggs, N_PIPE) == sum(int(m) for m, k in zip(meas, good) if k)
    out, mask, start = pw.agg_inputs()
    ints = [int(x) % P for x in out]
    assert int.from_bytes(o["agg_all"].tobytes(), "little") == (int(start[0]) + sum(ints)) % P
    assert int.from_bytes(o["agg_masked"].tobytes(), "little") == (int(start[0]) + sum(x for x, m in zip(ints, mask) if m)) % P
    assert o["guards"].all()      # nothing was written before or behind an output


def test_pipeline_default_run_takes_the_checks(pipe):
    _check_pipeline_run(pipe, pipe)


@pytest.mark.parametrize("env,device", [({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1),
                                        ({"CIRCL_HIP_ZEROCOPY_KB": "0"}, 0)], ids=["chunks", "chunks-in-shards", "merged-copy"])
def test_pipeline_routes_agree(pipe, tmp_path, env, device):
    import os
    import subprocess
    import sys
    import prio3_worker as pw
    dst = str(tmp_path / "out.npz")
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e.update(env)
    subprocess.run([sys.executable, os.path.abspath(pw.__file__), str(device), str(N_PIPE), dst], check=True, env=e, timeout=300)
    _check_pipeline_run(np.load(dst), pipe)
