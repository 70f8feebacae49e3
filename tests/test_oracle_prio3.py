"""The plain-Python Prio3 checker (tests/prio3.py) against the reference's Prio3Count / Prio3Sum vectors and its XofTurboShake128
vector (tests/golden/prio3.json.gz), and on measurements that are not valid."""
import gzip
import json
import os

import pytest

import prio3

HERE = os.path.dirname(os.path.abspath(__file__))
with gzip.open(os.path.join(HERE, "golden", "prio3.json.gz")) as _f:
    GOLDEN = json.load(_f)
FILES = sorted(GOLDEN["files"])


def task_of(v):
    return prio3.Task(v["kind"], v["max_measurement"], v["shares"], bytes.fromhex(v["ctx"]))


def test_fixture_is_whole():
    assert len(FILES) == 6 and sum(len(GOLDEN["files"][f]["prep"]) for f in FILES) == 17


def test_xof_vector():
    x = GOLDEN["xof"]
    got = prio3.xof(bytes.fromhex(x["seed"]), bytes.fromhex(x["dst"]), bytes.fromhex(x["binder"]), 32)
    assert got.hex() == x["derived_seed"]


@pytest.mark.parametrize("name", FILES)
def test_vectors(name):
    v = GOLDEN["files"][name]
    t = task_of(v)
    vk = bytes.fromhex(v["verify_key"])
    agg = [bytes(8)] * t.shares
    for p in v["prep"]:
        rand, nonce = bytes.fromhex(p["rand"]), bytes.fromhex(p["nonce"])
        leader = t.shard(p["measurement"], rand)
        shares = [leader] + [rand[32 * j:32 * j + 32] for j in range(t.shares - 1)]
        assert [s.hex() for s in shares] == p["input_shares"]
        preps = []
        for j in range(t.shares):
            ps, out = t.prep_init(j, vk, nonce, shares[j])
            assert ps.hex() == p["prep_shares"][0][j]
            assert [out.hex()] == p["out_shares"][j]
            preps.append(ps)
            agg[j] = prio3.aggregate(agg[j], [out])
        assert t.prep_finish(b"".join(preps))
    assert [a.hex() for a in agg] == v["agg_shares"]
    assert t.unshard(agg, len(v["prep"])) == v["agg_result"]


def flow_ok(t, meas, seed=1):
    rand = bytes((seed + 7 * i) & 255 for i in range(t.rand_size))
    vk, nonce = bytes(range(32)), bytes(range(16))
    leader = t.shard_encoded(meas, rand)
    shares = [leader] + [rand[32 * j:32 * j + 32] for j in range(t.shares - 1)]
    return t.prep_finish(b"".join(t.prep_init(j, vk, nonce, shares[j])[0] for j in range(t.shares)))


def test_rejects_what_is_not_a_bit():
    c = prio3.Task(prio3.COUNT, 0, 2, b"ctx")
    assert flow_ok(c, [0]) and flow_ok(c, [1]) and not flow_ok(c, [2])
    with pytest.raises(prio3.Prio3Error):
        c.encode(2)
    s = prio3.Task(prio3.SUM, 5, 3, b"ctx")
    assert flow_ok(s, s.encode(5)) and flow_ok(s, s.encode(0))
    bad = s.encode(3)
    bad[1] = 2
    assert not flow_ok(s, bad)


def test_rejects_a_sum_above_the_maximum():
    s = prio3.Task(prio3.SUM, 5, 2, b"ctx")
    with pytest.raises(prio3.Prio3Error):
        s.encode(6)
    # the bits of 6, with a second half that is the bits of 6 + offset: every element is a bit, the range check fails
    bad = [(6 >> i) & 1 for i in range(3)] + [((6 + s.offset) >> i) & 1 for i in range(3)]
    assert not flow_ok(s, bad)
    with pytest.raises(prio3.Prio3Error):
        prio3.Task(prio3.SUM, 2**62, 2, b"").unshard([bytes(8)] * 2, 8)


@pytest.mark.parametrize("bits,shares", [(1, 2), (2, 3), (3, 8), (4, 9), (32, 255), (63, 2)])
def test_self_consistent(bits, shares):
    t = prio3.Task(prio3.SUM, 2**bits - 1 if bits > 1 else 1, shares, b"some application")
    assert flow_ok(t, t.encode(t.max)) and flow_ok(t, t.encode(t.max // 3))
