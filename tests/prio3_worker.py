"""Child process of the Prio3 host-pipeline tests (tests/test_gpu_prio3.py): the pipeline's knobs (CIRCL_HIP_HOST_CHUNK,
CIRCL_HIP_ZEROCOPY_KB, CIRCL_HIP_LOGICAL_DEVICES) are read once per process, so every configuration needs a process of its own.

    python tests/prio3_worker.py DEVICE N OUT.npz

OUT gets what run() returns.  The parent calls run() itself for the default settings."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, kind, max_measurement, shares)
TASKS = (("count", 1, 0, 2), ("sum", 2, 1337, 3))
CTX = b"pipeline routes"
BAD = (7, 255, 256)            # measurements out of range: both sides of the chunk boundary 255 | 256 at CIRCL_HIP_HOST_CHUNK = 8
GUARD, FILL = 64, 0xA5
AGG_N = 3 * 4096 + 5           # three full rows of the host form's reduction and a tail


def inputs(name, n):
    kind, mx, shares = next(t[1:] for t in TASKS if t[0] == name)
    rng = np.random.default_rng(kind * 100 + n)
    meas = rng.integers(0, mx + 1 if kind == 2 else 2, n, dtype=np.uint64)
    for i in BAD:
        if i < n:
            meas[i] = mx + 1 if kind == 2 else 2
    return meas, rng.integers(0, 256, (n, 32 * shares), dtype=np.uint8), rng.integers(0, 256, (n, 16), dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)


def agg_inputs():
    rng = np.random.default_rng(4096)
    out = rng.integers(0, 2**64 - 2**32, AGG_N, dtype=np.uint64)
    return out, (rng.integers(0, 3, AGG_N) != 0).astype(np.uint8), rng.integers(0, 2**63, 1, dtype=np.uint64)


def run(L, device, n):
    """per task: shard, prep_init of every aggregator, prep_finish, aggregate of every aggregator's out shares under the verdicts; then one
    aggregate over AGG_N out shares with and without a mask.  Every output lies between guard margins; `guards` = every margin still
    holds its fill value."""
    from circl_amd import _native as nat
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    held, o = [], {}

    def guarded(nbytes):
        buf = np.full(nbytes + 2 * GUARD, FILL, np.uint8)
        held.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    for name, kind, mx, shares in TASKS:
        task = (kind, mx, shares, CTX, len(CTX))
        meas, rand, nonce, vk = inputs(name, n)
        ls, ps = L.circl_hip_prio3_leader_share_size(kind, mx), L.circl_hip_prio3_prep_share_size(kind)
        leader, ok = guarded(n * ls), guarded(n)
        nat.check(L.circl_hip_prio3_shard(*task, p(meas), p(rand), p(leader), p(ok), n, device), "prio3_shard")
        preps, verdict = guarded(n * shares * ps), guarded(n)
        rows = preps.reshape(n, shares, ps)
        for j in range(shares):
            share = leader if j == 0 else np.ascontiguousarray(rand[:, 32 * (j - 1):32 * j])
            prep, out, pok = guarded(n * ps), guarded(n * 8), guarded(n)
            nat.check(L.circl_hip_prio3_prep_init(*task, j, p(vk), p(nonce), p(share), p(prep), p(out), p(pok), n, device), "prio3_prep_init")
            rows[:, j, :] = prep.reshape(n, ps)
            o["%s_out%d" % (name, j)], o["%s_pok%d" % (name, j)] = out.copy(), pok.copy()
        nat.check(L.circl_hip_prio3_prep_finish(*task, p(preps), p(verdict), n, device), "prio3_prep_finish")
        for j in range(shares):
            agg = guarded(8)
            agg[:] = 0
            nat.check(L.circl_hip_prio3_aggregate(*task, p(o["%s_out%d" % (name, j)]), p(verdict), p(agg), n, device), "prio3_aggregate")
            o["%s_agg%d" % (name, j)] = agg.copy()
        o[name + "_leader"], o[name + "_ok"], o[name + "_preps"], o[name + "_verdict"] = leader.copy(), ok.copy(), preps.copy(), verdict.copy()
    out, mask, start = agg_inputs()
    for k, m in (("agg_all", None), ("agg_masked", mask)):
        agg = guarded(8)
        agg[:] = start.view(np.uint8)
        nat.check(L.circl_hip_prio3_aggregate(1, 0, 2, CTX, len(CTX), p(out), p(m), p(agg), AGG_N, device), "prio3_aggregate")
        o[k] = agg.copy()
    o["guards"] = np.array([(b[:GUARD] == FILL).all() and (b[GUARD + nb:] == FILL).all() for b, nb in held])
    return o


def main(device, n, dst):
    from circl_amd import _native as nat
    np.savez(dst, **run(nat.lib(), int(device), int(n)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
