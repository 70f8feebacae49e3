"""The host twins of tests/test_gpu_prio3_edges.py: the same inputs (tests/prio3_edges.py) through the device source compiled for the
host (tests/hostsim/prio3_hostsim.hip), bytewise against the checker -- seeds that make the rejection sampler refuse a word of a real
stream, contexts across the sponge's block edge, and field elements at the edges of fp64's reduction.

Two refusals in a row (2^-64) and the sampler's giving up after ten stay with the fake word source of tests/test_prio3_hostsim.py."""
import pytest

import prio3_edges as pe
from test_prio3_hostsim import Sim, hs  # noqa: F401  (hs: the fixture)


# ---- A: the sampler refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pe.RARE_BATCHES))
def test_a_lane_whose_sampler_refuses(hs, name):
    t, vk, meas, rands, nonces, placed, leaders, preps = pe.rare_batch(name)
    assert placed and all(c in pe.HITS for cs in placed.values() for c in cs)
    s, n = Sim(hs, t), len(meas)
    got, ok = s.shard(meas, rands)
    assert ok == [1] * n
    assert got == leaders, [i for i in range(n) if got[i] != leaders[i]]
    rows = [b""] * n
    for j in range(2):
        prep, out, ok = s.prep_init(j, vk, nonces, leaders if j == 0 else [r[:32] for r in rands])
        assert ok == [1] * n
        assert list(zip(prep, out)) == preps[j], (j, [i for i in range(n) if (prep[i], out[i]) != preps[j][i]])
        rows = [a + b for a, b in zip(rows, prep)]
    assert s.prep_finish(rows) == [1] * n


# ---- B: contexts across the block edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", pe.CTX_LENS)
@pytest.mark.parametrize("kind,mx", pe.CTX_TASKS)
def test_context_lengths(hs, kind, mx, length):
    t, vk, meas, rands, nonces, leaders, sent, preps, verdicts = pe.ctx_case(kind, mx, length)
    s, n = Sim(hs, t), pe.CTX_N
    got, ok = s.shard(meas, rands)
    assert ok == [1] * n and got == leaders
    rows = [b""] * n
    for j in range(2):
        prep, out, ok = s.prep_init(j, vk, nonces, sent if j == 0 else [r[:32] for r in rands])
        assert ok == [1] * n and list(zip(prep, out)) == preps[j], j
        rows = [a + b for a, b in zip(rows, prep)]
    assert s.prep_finish(rows) == verdicts


# ---- C: field elements at the reduction's edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mx,n", pe.LEADER_TASKS)
def test_leader_shares_of_edge_elements(hs, kind, mx, n):
    t, vk, nonces, rows, preps = pe.leader_case(kind, mx, n)
    prep, out, ok = Sim(hs, t).prep_init(0, vk, nonces, rows)
    assert ok == [1] * n
    assert list(zip(prep, out)) == preps, [i for i in range(n) if (prep[i], out[i]) != preps[i]]


@pytest.mark.parametrize("kind,mx,shares", pe.FINISH_TASKS)
def test_prep_shares_of_edge_elements(hs, kind, mx, shares):
    t, rows, verdicts = pe.finish_case(kind, mx, shares)
    got = Sim(hs, t).prep_finish(rows)
    assert got == verdicts, [i for i in range(len(rows)) if got[i] != verdicts[i]]
    assert 0 < sum(verdicts) < len(rows)
