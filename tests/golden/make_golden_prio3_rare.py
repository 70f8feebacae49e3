"""Writes tests/golden/prio3_rare.json.gz: seeds and nonces whose XofTurboShake128 streams make Prio3's rejection sampler refuse a
word (>= p, 2^-32 per word), found by oracle/prio3_search.c and checked here against the plain-Python checker tests/prio3.py.

    python tests/golden/make_golden_prio3_rare.py [--start COUNTER] [class ...]      (classes 1 .. 5, default all; minutes of CPU time)

Classes named on the command line are searched again (from --start, default class << 48); the others keep their entry in the file.
Candidates are LE64(counter) || 0x5c ... (oracle/orc.py prio3_candidate), so a run is reproducible.  Each class gets four times its
expected number of trials (a miss has probability e^-4) and is reported, not dropped, when it stays empty.

  class  task   searched                  stream that must refuse                       expected trials
  1      Sum    helper seed (agg_id 1)    measurement share, usage 1, words 0 .. 31     2^32 / 32
  2      Sum    helper seed (agg_id 1)    proof share, usage 2, words 0 .. 127          2^32 / 128
  3      Sum    helper seed (agg_id 1)    measurement share, word 20 (ends block 0)     2^32
  4      Sum    nonce, fixed verify key   query randomness, usage 5, words 0 .. 33      2^32 / 34
  5      Count  prove seed                prove randomness, usage 4, words 0 and 1      2^32 / 2
"""
import gzip
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import prio3  # noqa: E402
from oracle import orc  # noqa: E402

OUT = os.path.join(HERE, "prio3_rare.json.gz")
CTX = b"prio3 rare"
TASKS = {"sum": dict(kind=prio3.SUM, max_measurement=2**16 - 1, shares=2, ctx=CTX.hex()),
         "count": dict(kind=prio3.COUNT, max_measurement=0, shares=2, ctx=CTX.hex())}
VERIFY_KEY = bytes(range(0x40, 0x60))
# class: task, what the candidate is, usage, bytes between header and candidate, binder after it, candidate bytes, words looked at, block edge only
CLASSES = {1: ("sum", "helper_seed", 1, b"", bytes([1]), 32, 32, False),
           2: ("sum", "helper_seed", 2, b"", bytes([1, 1]), 32, 128, False),
           3: ("sum", "helper_seed", 1, b"", bytes([1]), 32, 21, True),
           4: ("sum", "nonce", 5, VERIFY_KEY + bytes([1]), b"", 16, 34, False),
           5: ("count", "prove_seed", 4, b"", bytes([1]), 32, 2, False)}


def task(name):
    t = TASKS[name]
    return prio3.Task(t["kind"], t["max_measurement"], t["shares"], bytes.fromhex(t["ctx"]))


def search(cls, start):
    name, what, usage, mid, binder, candlen, nwords, edge = CLASSES[cls]
    t = task(name)
    dst = bytes([12, 0]) + t.kind.to_bytes(4, "big") + usage.to_bytes(2, "big") + t.ctx
    pre = len(dst).to_bytes(2, "little") + dst + bytes([prio3.SEED]) + mid
    expected = 2**32 // (1 if edge else nwords)
    t0 = time.time()
    counter, index, perms = orc.prio3_search(pre, binder, candlen, start, 4 * expected, nwords, edge, 16)
    dt = time.time() - t0
    if counter is None:
        print("class %d: EMPTY after %d trials from counter %d (%d permutations, %.0f s); restart it with another --start" % (cls, 4 * expected, start, perms, dt))
        return None
    cand = orc.prio3_candidate(counter, candlen)
    # the checker's view of the same stream: seed and binder in the checker's terms
    seed, bind = (VERIFY_KEY, bytes([1]) + cand) if what == "nonce" else (cand, binder)
    words = t.stream(usage, seed, bind, 8 * (index + 1))
    w = [int.from_bytes(words[i:i + 8], "little") for i in range(0, len(words), 8)]
    assert w[index] >= prio3.P and all(x < prio3.P for k, x in enumerate(w[:index]) if not edge or k % 21 == 20), "the checker disagrees"
    print("class %d: counter %d (%d trials), word %d, %d permutations, %.0f s" % (cls, counter, counter - start + 1, index, perms, dt))
    return dict(cls=cls, task=name, what=what, value=cand.hex(), usage=usage, binder=bind.hex(), index=index, word="%016x" % w[index],
                counter=counter, start=start, trials=counter - start + 1, permutations=perms)


def main(argv):
    start = None
    if argv[:1] == ["--start"]:
        start, argv = int(argv[1], 0), argv[2:]
    todo = [int(a) for a in argv] or sorted(CLASSES)
    hits = {}
    if os.path.exists(OUT):
        with gzip.open(OUT) as f:
            hits = {h["cls"]: h for h in json.load(f)["hits"]}
    for cls in todo:
        h = search(cls, cls << 48 if start is None else start)
        if h is not None:
            hits[cls] = h
        out = {"tasks": TASKS, "verify_key": VERIFY_KEY.hex(), "hits": [hits[c] for c in sorted(hits)]}
        with gzip.GzipFile(OUT, "wb", mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode())
    missing = sorted(set(CLASSES) - set(hits))
    if missing:
        sys.exit("classes without a hit: %s" % missing)


if __name__ == "__main__":
    main(sys.argv[1:])
