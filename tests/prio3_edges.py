"""Inputs and expected outputs for Prio3's rare paths, shared by the GPU tests (test_gpu_prio3_edges.py) and their host twins
(test_prio3_edges_hostsim.py), so that both tiers run the same bytes.  TEST INFRASTRUCTURE ONLY.  Everything expected comes from the
plain-Python checker tests/prio3.py, computed once per case and cached.

  A  seeds and nonces that make the rejection sampler refuse a word (tests/golden/prio3_rare.json.gz), placed in batches of ordinary ones
  B  contexts that carry the XOF's message across the sponge's block edge
  C  field elements at the edges of fp64's reduction, as leader shares, prep shares and out shares
"""
import functools
import gzip
import json
import os
import random

import prio3

P = prio3.P
HERE = os.path.dirname(os.path.abspath(__file__))
with gzip.open(os.path.join(HERE, "golden", "prio3_rare.json.gz")) as _f:
    RARE = json.load(_f)
RARE_VK = bytes.fromhex(RARE["verify_key"])
HITS = {h["cls"]: h for h in RARE["hits"]}
CLASSES = (1, 2, 3, 4, 5)
SEARCH_PAD = 0x5c   # a candidate is LE64(counter) || SEARCH_PAD ... (oracle/prio3_search.c)


def rare_task(name):
    t = RARE["tasks"][name]
    return prio3.Task(t["kind"], t["max_measurement"], t["shares"], bytes.fromhex(t["ctx"]))


# ---- A: the sampler's refusals ------------------------------------------------------------------------------------------------------
def streams(t, rand, vk, nonce):
    """every stream that Shard and PrepInit (all aggregators) sample for one report: (name, usage, seed, binder, elements)"""
    out = [("prove", 4, rand[-32:], bytes([1]), t.arity), ("query", 5, vk, bytes([1]) + nonce, t.query_rand_len)]
    for j in range(1, t.shares):
        seed = rand[32 * (j - 1):32 * j]
        out += [("meas%d" % j, 1, seed, bytes([j]), t.meas_len), ("proof%d" % j, 2, seed, bytes([1, j]), t.proof_len)]
    return out


def refusals(t, rand, vk, nonce):
    """(stream, index) of every word >= p that one of the report's samplers reads"""
    found = []
    for name, usage, seed, binder, count in streams(t, rand, vk, nonce):
        s = t.stream(usage, seed, binder, 8 * (count + 16))
        got = k = 0
        while got < count:
            if int.from_bytes(s[8 * k:8 * k + 8], "little") >= P:
                found.append((name, k))
            else:
                got += 1
            k += 1
    return found


HIT_STREAM = {1: "meas1", 2: "proof1", 3: "meas1", 4: "query", 5: "prove"}   # the stream of `refusals` that a class makes refuse
# name: task, batch size, {lane: the classes placed there}.  Classes 1 to 3 are helper seeds, 4 a nonce, 5 a prove seed: a lane can
# carry a seed and the nonce.  The other lanes are ordinary.
RARE_BATCHES = {
    "sum130": ("sum", 130, {0: (1,), 1: (3, 4), 63: (2,), 64: (3,), 65: (2, 4), 128: (1,), 129: (4,)}),
    "count130": ("count", 130, {0: (5,), 63: (5,), 64: (5,), 129: (5,)}),
    "sum64": ("sum", 64, {37: (2,)}),      # one lane leaves a full wavefront
    "sum1": ("sum", 1, {0: (3,)}),
}


def _measurements(rng, t, n):
    meas = [rng.randrange(t.max + 1) if t.kind == prio3.SUM else rng.randrange(2) for _ in range(n)]
    meas[0], meas[-1] = (t.max, 0) if t.kind == prio3.SUM else (1, 0)
    return meas


def _flow(t, vk, meas, rands, nonces, sent=None):
    """the checker's leader shares, and (prep share, out share) per aggregator and report for the leader shares `sent`"""
    leaders = [t.shard(m, r) for m, r in zip(meas, rands)]
    sent = sent or leaders
    preps = {j: [t.prep_init(j, vk, nonces[i], sent[i] if j == 0 else rands[i][32 * (j - 1):32 * j]) for i in range(len(meas))] for j in range(t.shares)}
    return leaders, preps


@functools.lru_cache(maxsize=None)
def rare_batch(name):
    """-> t, vk, meas, rands, nonces, placed, leaders, preps"""
    task, n, placed = RARE_BATCHES[name]
    t = rare_task(task)
    rng = random.Random("rare " + name)
    rands, nonces = [rng.randbytes(t.rand_size) for _ in range(n)], [rng.randbytes(16) for _ in range(n)]
    for lane, classes in placed.items():
        for c in classes:
            v = bytes.fromhex(HITS[c]["value"])
            if c == 4:
                nonces[lane] = v
            elif c == 5:
                rands[lane] = rands[lane][:-32] + v
            else:
                rands[lane] = v + rands[lane][32:]
    meas = _measurements(rng, t, n)
    leaders, preps = _flow(t, RARE_VK, meas, rands, nonces)
    return t, RARE_VK, meas, rands, nonces, placed, leaders, preps


# ---- B: contexts across the block edge --------------------------------------------------------------------------------------------
# The message is header || seed || binder [|| nonce]: 44 + ctx bytes (prove randomness, measurement share), 45 + ctx (proof share),
# 60 + ctx (query randomness) against a rate of 168.  107 / 108: the query randomness at 167 (the domain byte and the final bit share
# byte 167) and 168 (a second block that holds only the domain byte); 122 / 123 / 124: the other three at 166 to 168; 255: the longest.
CTX_LENS = (0, 107, 108, 122, 123, 124, 255)
CTX_TASKS = ((prio3.COUNT, 0), (prio3.SUM, 255))
CTX_N = 65
CTX_CHEAT = 3   # this report's leader share comes from a cheating client, so that the verdicts are not all alike


@functools.lru_cache(maxsize=None)
def ctx_case(kind, mx, length):
    """-> t, vk, meas, rands, nonces, leaders, sent, preps, verdicts"""
    rng = random.Random("ctx %d %d" % (kind, length))
    t = prio3.Task(kind, mx, 2, rng.randbytes(length))
    vk = rng.randbytes(32)
    rands, nonces = [rng.randbytes(t.rand_size) for _ in range(CTX_N)], [rng.randbytes(16) for _ in range(CTX_N)]
    meas = _measurements(rng, t, CTX_N)
    enc = t.encode(meas[CTX_CHEAT])
    enc[0] = 2
    sent = [t.shard_encoded(enc, r) if i == CTX_CHEAT else t.shard(m, r) for i, (m, r) in enumerate(zip(meas, rands))]
    leaders, preps = _flow(t, vk, meas, rands, nonces, sent)
    verdicts = [int(t.prep_finish(preps[0][i][0] + preps[1][i][0])) for i in range(CTX_N)]
    assert verdicts == [int(i != CTX_CHEAT) for i in range(CTX_N)]
    return t, vk, meas, rands, nonces, leaders, sent, preps, verdicts


# ---- C: field elements at the reduction's edges --------------------------------------------------------------------------------------
# fp64 folds a carry or a borrow back with +- (2^32 - 1): the elements around 2^32, around p, and the multiples of 2^32 (a zero low
# word, which is what reduce128's `lo < hh` borrow needs: 2^63 * 2^k has lo = 0 and hh = 2^(k - 33) for k >= 33)
EDGE = [0, 1, 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**63 + 2**32, 3 * 2**32, (2**31 - 1) * 2**32, (2**32 - 2) * 2**32, (P - 1) // 2, (P + 1) // 2,
        P - 2**32, P - 2, P - 1]
assert all(0 <= e < P for e in EDGE) and len(set(EDGE)) == len(EDGE) == 16
LEADER_TASKS = ((prio3.SUM, 2**63 - 1, 130), (prio3.SUM, 2**40 - 1, 97), (prio3.SUM, 2**34 - 1, 66), (prio3.COUNT, 0, 65))   # kind, max, n


@functools.lru_cache(maxsize=None)
def leader_case(kind, mx, n):
    """Leader shares made of edge elements (they prove nothing: PrepInit computes a verifier share for any canonical row).
    Rows 0 .. 15 and 16 .. 31 cycle every element of EDGE through every position of the row, in two orders; then one row per bit
    position k = 33 .. bits - 1 with 2^63 at k in both halves of the measurement (CircuitSum::on_meas multiplies it by 2^k); then
    random draws from EDGE; the last two rows are all 2^63 and all p - 1.  -> t, vk, nonces, rows, preps (agg_id 0)"""
    rng = random.Random("leader edges %d %d" % (kind, mx))
    t = prio3.Task(kind, mx, 2, b"field edges")
    vk, nonces = rng.randbytes(32), [rng.randbytes(16) for _ in range(n)]
    words, E = t.meas_len + t.proof_len, len(EDGE)
    rows = [[EDGE[(i + j) % E] for j in range(words)] for i in range(E)] + [[EDGE[(5 * i + 3 * j) % E] for j in range(words)] for i in range(E)]
    for k in range(33, t.bits):
        row = [rng.choice(EDGE) for _ in range(words)]
        row[k] = row[t.bits + k] = 2**63
        rows.append(row)
    assert len(rows) <= n - 2
    rows += [[rng.choice(EDGE) for _ in range(words)] for _ in range(n - 2 - len(rows))]
    rows += [[2**63] * words, [P - 1] * words]
    rows = [prio3.enc(r) for r in rows]
    return t, vk, nonces, rows, [t.prep_init(0, vk, nonces[i], rows[i]) for i in range(n)]


FINISH_TASKS = ((prio3.COUNT, 0, 2), (prio3.COUNT, 0, 255), (prio3.SUM, 255, 2), (prio3.SUM, 255, 255))   # kind, max, shares


@functools.lru_cache(maxsize=None)
def finish_case(kind, mx, shares):
    """Rows of prep shares for PrepSharesToPrep: the elements of EDGE cycled through every position; every element equal to one edge
    element (255 times p - 1 among them); rows that verify -- real reports (and a cheating one) of a two-share task, for more shares
    padded with edge elements and one balancing share, which leaves the sum alone -- and rows of edge elements whose last share
    balances them to an accepting verifier.  (max = 255 has offset 0, so the verifier's sum does not depend on the share count.)
    -> t, rows, verdicts"""
    rng = random.Random("finish edges %d %d" % (kind, shares))
    t = prio3.Task(kind, mx, shares, b"field edges")
    V, E = t.verifier_len, len(EDGE)
    rows = [[EDGE[(i + j) % E] for j in range(shares * V)] for i in range(E)] + [[e] * (shares * V) for e in EDGE]

    def balanced(fill, total):
        """shares - 1 shares `fill` and a last one that brings the sum to `total`"""
        last = [(total[k] - sum(fill[j * V + k] for j in range(shares - 1))) % P for k in range(V)]
        return fill + last

    t2 = prio3.Task(kind, mx, 2, b"field edges")
    vk, n2 = rng.randbytes(32), 8
    rands, nonces = [rng.randbytes(t2.rand_size) for _ in range(n2)], [rng.randbytes(16) for _ in range(n2)]
    meas = _measurements(rng, t2, n2)
    enc = t2.encode(meas[2])
    enc[0] = 2
    sent = [t2.shard_encoded(enc, r) if i == 2 else t2.shard(m, r) for i, (m, r) in enumerate(zip(meas, rands))]
    _, preps = _flow(t2, vk, meas, rands, nonces, sent)
    for i in range(n2):
        a, b = prio3.dec(preps[0][i][0]), prio3.dec(preps[1][i][0])
        rows.append(balanced(a + [rng.choice(EDGE) for _ in range((shares - 2) * V)], [(x + y) % P for x, y in zip(a, b)]))
    for w in EDGE:
        wires = [w] * t.arity if kind == prio3.SUM else [w, EDGE[(EDGE.index(w) + 5) % E]]
        fill = [rng.choice(EDGE) for _ in range((shares - 1) * V)]
        rows.append(balanced(fill, [0] + wires + [t.gadget(wires)]))                     # accepted
        rows.append(balanced(fill, [0] + wires + [(t.gadget(wires) + 1) % P]))           # the gadget check fails by one
        rows.append(balanced(fill, [P - 1] + wires + [t.gadget(wires)]))                 # the circuit's output is p - 1, not 0
    rows = [prio3.enc(r) for r in rows]
    verdicts = [int(t.prep_finish(r)) for r in rows]
    assert verdicts[2 * E:2 * E + n2] == [1, 1, 0] + [1] * (n2 - 3) and verdicts[2 * E + n2:] == [1, 0, 0] * E
    return t, rows, verdicts


AGG_SIZES = (65, 4097)


def aggregate_cases(n):
    """(start, out shares) for AggregateUpdate: every out share p - 1; draws from EDGE; each with a start value from EDGE"""
    rng = random.Random("aggregate edges %d" % n)
    cases = [(P - 1, [P - 1] * n), (2**32, [P - 1] * n)]
    cases += [(EDGE[(7 * k + n) % len(EDGE)], [EDGE[(i + k) % len(EDGE)] if k < 2 else rng.choice(EDGE) for i in range(n)]) for k in range(4)]
    return cases
