"""The device source of Prio3Count / Prio3Sum (circl_amd/csrc/prio3_kernels.h, prio3_xof_dev.h, fp64_dev.h) compiled for the host
(tests/hostsim/prio3_hostsim.hip): the item functions on the reference's vectors and against the checker, Field64 against Python's
integers, the transforms against naive evaluation, and the paths no seed can be aimed at -- the sampler's rejections, its giving up, an
evaluation point that is a root of unity -- at the function."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import prio3
from test_oracle_prio3 import FILES, GOLDEN, task_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "prio3_hostsim.hip")
vp = C.c_void_p
P = prio3.P


def _stale(out):
    from circl_amd import build
    deps = [SRC] + [os.path.join(build.CSRC, h) for h in ("prio3_kernels.h", "prio3_xof_dev.h", "fp64_dev.h", "keccak_dev.h")]
    return not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in deps)


def _hipcc(out, *flags):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "circl_amd", "csrc"), *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def hs():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "build", "libprio3_hostsim.so"), "-shared", "-fPIC"))
    lib.hs_prio3_task_size.restype = C.c_size_t
    lib.hs_prio3_task.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t, vp]
    lib.hs_prio3_sizes.argtypes = [vp, vp]
    lib.hs_prio3_shard.argtypes = [vp, C.c_size_t, vp, vp, vp, vp]
    lib.hs_prio3_prep_init.argtypes = [vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    lib.hs_prio3_prep_finish.argtypes = [vp, C.c_size_t, vp, vp]
    lib.hs_prio3_query.argtypes = [vp, vp, vp, vp, vp]
    lib.hs_fp64.argtypes = [C.c_int, vp, vp, vp, C.c_size_t]
    lib.hs_prio3_ntt.argtypes = [C.c_uint32, vp, C.c_int]
    lib.hs_prio3_sample.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.hs_prio3_sample.restype = C.c_size_t
    return lib


def _p(a):
    return a.ctypes.data_as(vp)


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


class Sim:
    """the operations of the ABI over batches, through the host instantiation"""

    def __init__(self, hs, t):
        self.hs, self.t = hs, t
        self.task = np.zeros(hs.hs_prio3_task_size(), np.uint8)
        assert hs.hs_prio3_task(t.kind, t.max, t.shares, t.ctx, len(t.ctx), _p(self.task)) == 0
        sizes = np.zeros(5, np.uint32)
        hs.hs_prio3_sizes(_p(self.task), _p(sizes))
        self.leader_words, self.verifier_len, self.ws_elems, self.p, self.query_rand_len = (int(x) for x in sizes)

    def shard(self, measurements, rands):
        n = len(measurements)
        m, r = np.array(measurements, np.uint64), _u8(b"".join(rands))
        leader, ok = np.full(n * self.leader_words, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(n, 7, np.uint8)
        self.hs.hs_prio3_shard(_p(self.task), n, _p(m), _p(r), _p(leader), _p(ok))
        b = leader.tobytes()
        return [b[i * 8 * self.leader_words:(i + 1) * 8 * self.leader_words] for i in range(n)], list(ok)

    def prep_init(self, agg_id, verify_key, nonces, shares):
        n = len(nonces)
        vk, nn = _u8(verify_key), _u8(b"".join(nonces))
        sh = np.frombuffer(b"".join(shares), np.uint64).copy()
        prep, out, ok = np.full(n * self.verifier_len, 0xA5, np.uint64), np.full(n, 0xA5, np.uint64), np.full(n, 7, np.uint8)
        self.hs.hs_prio3_prep_init(_p(self.task), agg_id, _p(vk), n, _p(nn), _p(sh), _p(prep), _p(out), _p(ok))
        pb, ob, k = prep.tobytes(), out.tobytes(), 8 * self.verifier_len
        return [pb[i * k:(i + 1) * k] for i in range(n)], [ob[8 * i:8 * i + 8] for i in range(n)], list(ok)

    def prep_finish(self, rows):
        ps, ok = np.frombuffer(b"".join(rows), np.uint64).copy(), np.full(len(rows), 7, np.uint8)
        self.hs.hs_prio3_prep_finish(_p(self.task), len(rows), _p(ps), _p(ok))
        return list(ok)


def test_sizes(hs):
    for b, p in [(1, 4), (2, 8), (3, 8), (4, 16), (7, 16), (8, 32), (15, 32), (16, 64), (31, 64), (32, 128), (63, 128)]:
        s = Sim(hs, prio3.Task(prio3.SUM, 2**b - 1, 2, b""))
        assert (s.p, s.leader_words, s.verifier_len, s.query_rand_len) == (p, 2 * b + 2 * p, 3, 2 * b + 2)
    s = Sim(hs, prio3.Task(prio3.COUNT, 0, 2, b""))
    assert (s.p, s.leader_words, s.verifier_len, s.query_rand_len) == (2, 6, 4, 2)


@pytest.mark.parametrize("name", FILES)
def test_whole_fixture(hs, name):
    v = GOLDEN["files"][name]
    t = task_of(v)
    s = Sim(hs, t)
    vk = bytes.fromhex(v["verify_key"])
    rands = [bytes.fromhex(p["rand"]) for p in v["prep"]]
    nonces = [bytes.fromhex(p["nonce"]) for p in v["prep"]]
    leaders, ok = s.shard([p["measurement"] for p in v["prep"]], rands)
    assert ok == [1] * len(rands)
    assert [x.hex() for x in leaders] == [p["input_shares"][0] for p in v["prep"]]
    rows = [b""] * len(rands)
    for j in range(t.shares):
        shares = leaders if j == 0 else [r[32 * (j - 1):32 * j] for r in rands]
        prep, out, ok = s.prep_init(j, vk, nonces, shares)
        assert ok == [1] * len(rands)
        assert [x.hex() for x in prep] == [p["prep_shares"][0][j] for p in v["prep"]]
        assert [[x.hex()] for x in out] == [p["out_shares"][j] for p in v["prep"]]
        rows = [a + b for a, b in zip(rows, prep)]
    assert s.prep_finish(rows) == [1] * len(rands)


@pytest.mark.parametrize("kind,mx,shares", [(1, 0, 2), (1, 0, 9), (2, 1, 2), (2, 2, 3), (2, 7, 8), (2, 8, 9), (2, 1337, 3), (2, 2**31, 2), (2, 2**63 - 1, 2), (2, 255, 255)])
def test_against_the_checker_with_bad_items(hs, kind, mx, shares):
    """a measurement out of range, a leader share and a prep share that are not canonical, a flipped proof byte, a cheating client"""
    rng = random.Random(kind * 1000 + mx % 997 + shares)
    t = prio3.Task(kind, mx, shares, b"checker ctx")
    s = Sim(hs, t)
    n = 6
    vk = rng.randbytes(32)
    rands, nonces = [rng.randbytes(t.rand_size) for _ in range(n)], [rng.randbytes(16) for _ in range(n)]
    meas = [rng.randrange(mx + 1) if kind == 2 else rng.randrange(2) for _ in range(n)]
    meas[1] = mx + 1 if kind == 2 else 2
    leaders, ok = s.shard(meas, rands)
    assert ok == [1, 0, 1, 1, 1, 1] and leaders[1] == bytes(len(leaders[1]))
    for i in (0, 2, 3, 4, 5):
        assert leaders[i] == t.shard(meas[i], rands[i])
    leaders[1] = t.shard(0, rands[1])
    leaders[2] = leaders[2][:8] + (P + 1).to_bytes(8, "little") + leaders[2][16:]                 # not canonical
    leaders[3] = leaders[3][:-3] + bytes([leaders[3][-3] ^ 0x10]) + leaders[3][-2:]               # a flipped proof byte
    cheat = t.encode(meas[4])
    cheat[0] = 2
    leaders[4] = t.shard_encoded(cheat, rands[4])                                                # a client that cheats
    rows, outs = [b""] * n, []
    for j in sorted({0, 1, shares - 1} if shares != 3 else {0, 1, 2}):
        shares_j = leaders if j == 0 else [r[32 * (j - 1):32 * j] for r in rands]
        prep, out, ok = s.prep_init(j, vk, nonces, shares_j)
        for i in range(n):
            if j == 0 and i == 2:
                assert ok[i] == 0 and prep[i] == bytes(len(prep[i])) and out[i] == bytes(8)
                continue
            want = t.prep_init(j, vk, nonces[i], shares_j[i])
            assert ok[i] == 1 and (prep[i], out[i]) == want, (j, i)
    # every aggregator, through the checker for those not run above
    for i in range(n):
        ps = []
        for j in range(shares):
            try:
                ps.append(t.prep_init(j, vk, nonces[i], leaders[i] if j == 0 else rands[i][32 * (j - 1):32 * j])[0])
            except prio3.Prio3Error:
                ps.append(bytes(t.prep_share_size))
        rows[i] = b"".join(ps)
    rows[5] = rows[5][:16] + (2**64 - 1).to_bytes(8, "little") + rows[5][24:]                    # a prep share that is not canonical
    got = s.prep_finish(rows)
    assert got == [int(t.prep_finish(r)) for r in rows]
    assert got == [1, 1, 0, 0, 0, 0]


EDGES = [0, 1, P - 1, 2**32 - 1, 2**32, 2**64 - 2**32]


def test_field64(hs):
    rng = random.Random(64)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.randrange(P), rng.randrange(P)) for _ in range(4096)]
    a, b = np.array([x for x, _ in pairs], np.uint64), np.array([y for _, y in pairs], np.uint64)
    out = np.zeros_like(a)
    for op, f in enumerate([lambda x, y: (x + y) % P, lambda x, y: (x - y) % P, lambda x, y: x * y % P, lambda x, y: x * x % P, lambda x, y: pow(x, P - 2, P)]):
        hs.hs_fp64(op, _p(a), _p(b), _p(out), len(pairs))
        assert [int(x) for x in out] == [f(x, y) for x, y in pairs], op


@pytest.mark.parametrize("lg", range(1, 8))
def test_transform_against_naive_evaluation(hs, lg):
    rng = random.Random(lg)
    n = 1 << lg
    c = [rng.randrange(P) for _ in range(n)]
    c[0], c[-1] = P - 1, 2**32
    w = prio3.root(lg)
    v = np.array(c, np.uint64)
    hs.hs_prio3_ntt(lg, _p(v), 0)
    assert [int(x) for x in v] == [prio3.horner(c, pow(w, k, P)) for k in range(n)]
    hs.hs_prio3_ntt(lg, _p(v), 1)
    assert [int(x) for x in v] == c


def _sample(hs, words, count):
    w, out, used = np.array(words, np.uint64), np.zeros(count, np.uint64), C.c_size_t(0)
    k = hs.hs_prio3_sample(_p(w), len(words), _p(out), count, C.byref(used))
    return k, [int(x) for x in out[:k]], used.value


def test_sampler_skips_what_is_not_canonical(hs):
    assert _sample(hs, [P, P + 1, 2**64 - 1, P - 1, 5], 2) == (2, [P - 1, 5], 5)
    assert _sample(hs, [P] * 9 + [3, 4], 2) == (2, [3, 4], 11)


def test_sampler_gives_up_after_ten(hs):
    assert _sample(hs, [7] + [P] * 10 + [1], 2) == (1, [7], 11)


def test_query_refuses_a_root_of_unity(hs):
    for t in (prio3.Task(prio3.COUNT, 0, 2, b""), prio3.Task(prio3.SUM, 6, 2, b"")):
        s = Sim(hs, t)
        rng = random.Random(t.kind)
        share = np.array([rng.randrange(P) for _ in range(s.leader_words)], np.uint64)
        ti = 0 if t.kind == prio3.COUNT else t.eval_out
        for tt, want in [(pow(prio3.root(s.p.bit_length() - 1), 3, P), 0), (1, 0), (7, 1)]:
            qr = [rng.randrange(P) for _ in range(s.query_rand_len)]
            qr[ti] = tt
            rand, ver, out = np.array(qr, np.uint64), np.zeros(s.verifier_len, np.uint64), np.zeros(1, np.uint64)
            assert hs.hs_prio3_query(_p(s.task), _p(rand), _p(share), _p(ver), _p(out)) == want
            if want:
                meas, proof = [int(x) for x in share[:t.meas_len]], [int(x) for x in share[t.meas_len:]]
                assert [int(x) for x in ver] == t.query(meas, proof, qr)


def test_standalone_program_under_sanitizers():
    """the same source with its own main, host code instrumented: buffers of exactly their size"""
    exe = _hipcc(os.path.join(ROOT, "build", "prio3_hostsim_san"), "-DPRIO3_HOSTSIM_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "prio3_hostsim: ok" in r.stdout, r.stdout[-3000:]
