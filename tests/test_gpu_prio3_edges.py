"""Prio3Count / Prio3Sum on the GPU where no random input goes: a lane whose rejection sampler refuses a word (and so leaves its
wavefront's lockstep, at a block edge too), contexts that take the XOF's message across the sponge's block edge, and field elements at
the edges of fp64's reduction.  Both forms, bytewise against the checker tests/prio3.py, every output between sentinels.  The inputs
are tests/prio3_edges.py's, which tests/test_prio3_edges_hostsim.py runs through the host build of the same source.

The refusing seeds were searched for ahead of time (tests/golden/prio3_rare.json.gz).  Two refusals in a row (2^-64) and the sampler's
giving up after ten stay with the fake word source of tests/test_prio3_hostsim.py: no search reaches them."""
import numpy as np
import pytest

import prio3
import prio3_edges as pe
from test_gpu_prio3 import FORMS, Gpu, L  # noqa: F401  (L: the fixture)

pytestmark = pytest.mark.gpu
P = prio3.P


def whole_flow(g, t, vk, meas, rands, nonces, leaders, preps):
    """shard, prep_init for both aggregators, prep_finish, aggregate and unshard of a batch of good reports"""
    n = len(meas)
    got, ok = g.shard(meas, rands)
    assert ok == [1] * n
    assert got == leaders, [i for i in range(n) if got[i] != leaders[i]]
    rows, aggs = [b""] * n, []
    for j in range(2):
        prep, out, ok = g.prep_init(j, vk, nonces, leaders if j == 0 else [r[:32] for r in rands])
        assert ok == [1] * n
        assert list(zip(prep, out)) == preps[j], (j, [i for i in range(n) if (prep[i], out[i]) != preps[j][i]])
        rows = [a + b for a, b in zip(rows, prep)]
        aggs.append(g.aggregate(bytes(8), out))
        assert aggs[-1] == prio3.aggregate(bytes(8), out)
    assert g.prep_finish(rows) == [1] * n
    assert g.unshard(aggs, n) == sum(meas)


# ---- A: the sampler refuses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(pe.RARE_BATCHES))
def test_a_lane_whose_sampler_refuses(L, form, name):
    t, vk, meas, rands, nonces, placed, leaders, preps = pe.rare_batch(name)
    assert placed and all(c in pe.HITS for cs in placed.values() for c in cs)
    whole_flow(Gpu(L, form, t), t, vk, meas, rands, nonces, leaders, preps)


# ---- B: contexts across the block edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("length", pe.CTX_LENS)
@pytest.mark.parametrize("kind,mx", pe.CTX_TASKS)
def test_context_lengths(L, form, kind, mx, length):
    t, vk, meas, rands, nonces, leaders, sent, preps, verdicts = pe.ctx_case(kind, mx, length)
    g, n = Gpu(L, form, t), pe.CTX_N
    got, ok = g.shard(meas, rands)
    assert ok == [1] * n and got == leaders
    rows = [b""] * n
    for j in range(2):
        prep, out, ok = g.prep_init(j, vk, nonces, sent if j == 0 else [r[:32] for r in rands])
        assert ok == [1] * n and list(zip(prep, out)) == preps[j], j
        rows = [a + b for a, b in zip(rows, prep)]
    assert g.prep_finish(rows) == verdicts


@pytest.mark.parametrize("kind,mx", pe.CTX_TASKS)
def test_the_wrappers_take_the_longest_context(kind, mx):
    import torch
    from circl_amd import device as dev
    from circl_amd import hostapi as api
    t, vk, meas, rands, nonces, leaders, sent, preps, verdicts = pe.ctx_case(kind, mx, 255)
    n = pe.CTX_N
    h, d = api.Prio3(kind, mx, 2, t.ctx), dev.Prio3Device(kind, mx, 2, t.ctx)
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    rand_a, nonce_a = np.frombuffer(b"".join(rands), np.uint8).reshape(n, -1), np.frombuffer(b"".join(nonces), np.uint8).reshape(n, 16)
    sent_a = np.frombuffer(b"".join(sent), np.uint8).reshape(n, -1)
    lh, okh = h.shard(meas, rand_a)
    ld, okd = d.shard(cu(np.array(meas, np.int64)), cu(rand_a))
    assert okh.all() and okd.cpu().numpy().all()
    assert [r.tobytes() for r in lh] == leaders and (ld.cpu().numpy() == lh).all()
    rows_h = np.zeros((n, 2, t.prep_share_size), np.uint8)
    rows_d = torch.zeros((n, 2, t.prep_share_size), dtype=torch.uint8, device="cuda")
    for j in range(2):
        sh = sent_a if j == 0 else rand_a[:, :32]
        ph, oh, okh = h.prep_init(j, vk, nonce_a, sh)
        pd, od, okd = d.prep_init(j, cu(np.frombuffer(vk, np.uint8)), cu(nonce_a), cu(sh))
        assert okh.all() and okd.cpu().numpy().all()
        assert [(a.tobytes(), b.tobytes()) for a, b in zip(ph, oh)] == preps[j]
        assert (pd.cpu().numpy() == ph).all() and (od.cpu().numpy() == oh).all()
        rows_h[:, j], rows_d[:, j] = ph, pd
    assert [int(x) for x in h.prep_finish(rows_h)] == verdicts
    assert [int(x) for x in d.prep_finish(rows_d.contiguous()).cpu().numpy()] == verdicts


# ---- C: field elements at the reduction's edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,mx,n", pe.LEADER_TASKS)
def test_leader_shares_of_edge_elements(L, form, kind, mx, n):
    t, vk, nonces, rows, preps = pe.leader_case(kind, mx, n)
    prep, out, ok = Gpu(L, form, t).prep_init(0, vk, nonces, rows)
    assert ok == [1] * n
    assert list(zip(prep, out)) == preps, [i for i in range(n) if (prep[i], out[i]) != preps[i]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,mx,shares", pe.FINISH_TASKS)
def test_prep_shares_of_edge_elements(L, form, kind, mx, shares):
    t, rows, verdicts = pe.finish_case(kind, mx, shares)
    got = Gpu(L, form, t).prep_finish(rows)
    assert got == verdicts, [i for i in range(len(rows)) if got[i] != verdicts[i]]
    assert 0 < sum(verdicts) < len(rows)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", pe.AGG_SIZES)
def test_aggregate_of_edge_elements(L, form, n):
    g = Gpu(L, form, prio3.Task(prio3.COUNT, 0, 2, b""))
    for start, outs in pe.aggregate_cases(n):
        assert g.aggregate(start.to_bytes(8, "little"), np.array(outs, np.uint64)) == ((start + sum(outs)) % P).to_bytes(8, "little"), start
