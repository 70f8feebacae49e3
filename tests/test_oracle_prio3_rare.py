"""The rare-path fixture tests/golden/prio3_rare.json.gz (tests/golden/make_golden_prio3_rare.py) proved with the plain-Python checker
alone: every recorded seed or nonce makes the recorded stream refuse the recorded word, and in the batches of tests/prio3_edges.py only
the placed lanes refuse anywhere.  Nothing is searched here: the oracle's search routine is run over the few counters before a
recorded hit only.

Two refusals in a row (2^-64) and the sampler's giving up after ten are out of any search's reach; they stay with the fake word source
of tests/test_prio3_hostsim.py."""
import pytest

import prio3
import prio3_edges as pe
from oracle import orc

P = prio3.P
COUNTS = {1: ("sum", 1, 32), 2: ("sum", 2, 128), 3: ("sum", 1, 32), 4: ("sum", 5, 34), 5: ("count", 4, 2)}   # task, usage, elements of the stream


def test_every_class_has_a_hit():
    assert sorted(pe.HITS) == list(pe.CLASSES)
    s, c = pe.rare_task("sum"), pe.rare_task("count")
    assert (s.kind, s.max, s.shares, s.meas_len, s.p, s.proof_len, s.query_rand_len) == (prio3.SUM, 2**16 - 1, 2, 32, 64, 128, 34)
    assert (c.kind, c.shares, c.arity) == (prio3.COUNT, 2, 2) and len(s.ctx) <= 16 and s.ctx == c.ctx


@pytest.mark.parametrize("cls", pe.CLASSES)
def test_recorded_hit(cls):
    h = pe.HITS[cls]
    task, usage, count = COUNTS[cls]
    assert (h["task"], h["usage"]) == (task, usage)
    t = pe.rare_task(task)
    value = bytes.fromhex(h["value"])
    assert value == h["counter"].to_bytes(8, "little") + bytes([pe.SEARCH_PAD]) * (8 if cls == 4 else 24)
    assert h["start"] <= h["counter"] and h["trials"] == h["counter"] - h["start"] + 1
    seed, binder = (pe.RARE_VK, bytes([1]) + value) if cls == 4 else (value, bytes({1: [1], 2: [1, 1], 3: [1], 5: [1]}[cls]))
    assert h["binder"] == binder.hex()
    s = t.stream(usage, seed, binder, 8 * (count + 1))
    words = [int.from_bytes(s[i:i + 8], "little") for i in range(0, len(s), 8)]
    k = h["index"]
    assert k < count and words[k] >= P and "%016x" % words[k] == h["word"]
    if cls == 3:
        assert k % 21 == 20      # the last word of a squeezed block: the next read permutes
    else:
        assert all(w < P for w in words[:k])
    # the sampler reads one word more and yields the same elements as the stream without the refused words
    want = [w for w in words if w < P][:count]
    assert t.vec(usage, seed, binder, count) == want and len(want) == count


@pytest.mark.parametrize("name", sorted(pe.RARE_BATCHES))
def test_only_the_placed_lanes_refuse(name):
    t, vk, meas, rands, nonces, placed, leaders, preps = pe.rare_batch(name)
    for i in range(len(meas)):
        want = sorted((pe.HIT_STREAM[c], pe.HITS[c]["index"]) for c in placed.get(i, ()))
        assert sorted(pe.refusals(t, rands[i], vk, nonces[i])) == want, i
    # and the reports are good ones: the checker accepts every one of them
    assert all(t.prep_finish(preps[0][i][0] + preps[1][i][0]) for i in range(len(meas)))


def test_batches_place_every_class_at_the_wavefront_edges():
    for name, lanes in (("sum130", (0, 63, 64, 129)), ("count130", (0, 63, 64, 129))):
        _, n, placed = pe.RARE_BATCHES[name]
        assert n == 130 and all(placed.get(i) for i in lanes)
    assert {c for _, _, placed in pe.RARE_BATCHES.values() for cs in placed.values() for c in cs} == set(pe.CLASSES)
    assert pe.RARE_BATCHES["sum64"][1] == 64 and len(pe.RARE_BATCHES["sum64"][2]) == 1
    assert pe.RARE_BATCHES["sum1"] == ("sum", 1, {0: (3,)})


# ---- the search routine, over the counters just before a recorded hit ------------------------------------------------------------------
def _search_args(cls):
    h = pe.HITS[cls]
    task, usage, count = COUNTS[cls]
    t = pe.rare_task(task)
    dst = bytes([12, 0]) + t.kind.to_bytes(4, "big") + usage.to_bytes(2, "big") + t.ctx
    pre = len(dst).to_bytes(2, "little") + dst + bytes([prio3.SEED]) + (pe.RARE_VK + bytes([1]) if cls == 4 else b"")
    suf = b"" if cls == 4 else bytes.fromhex(h["binder"])
    return h, pre, suf, 16 if cls == 4 else 32, 21 if cls == 3 else count, cls == 3


@pytest.mark.parametrize("cls", pe.CLASSES)
def test_search_finds_the_recorded_hit_again(cls):
    h, pre, suf, candlen, nwords, edge = _search_args(cls)
    assert orc.prio3_candidate(h["counter"], candlen).hex() == h["value"]
    back = 200000
    for threads in (1, 3, 16):      # the answer does not depend on how the range is cut up
        assert orc.prio3_search(pre, suf, candlen, h["counter"] - back, back + 5, nwords, edge, threads)[:2] == (h["counter"], h["index"])
    counter, index, perms = orc.prio3_search(pre, suf, candlen, h["counter"] - back, back, nwords, edge, 16)
    assert (counter, index) == (None, None) and perms == back * ((nwords + 20) // 21)
