"""Coalesced and queued table calls AT their admission limits (host_coalesce.hip): whether a call joins a shared batch or runs on its own
is decided by admissible() (a quarter of the blob area, max_items / 4 items), by reserve() (a batch closes when the next call's items or
blob bytes would overflow it) and by what coalesce_run / coalesce_submit make of the two.  Here every one of those edges is met from both
sides, with ML-DSA-44 messages as the blob: a blocking call beyond the limit takes the pipeline (also on a table with a queue: only
*_submit refuses it), batches close on blob bytes before they close on items, rows of very different lengths share a batch, and a
caller's offsets need not start at zero (item i is msg_blob[msg_off[i] .. msg_off[i + 1]): a C or Go caller slicing one buffer).

Every comparison is bytewise against the oracle; there are no tolerances.  The limit itself is not taken on trust from the formula
restated below: the table's joined-calls counter (coalesce_stats()[0]) says whether a call joined a batch or ran alone.

(Contexts are the second blob and are counted on their own, but they cannot reach the quarter rule: call_max * 255 < Q for every max_items.)"""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAM, NKEYS, SIG = 44, 2, 2420
EPARAM = -1


def _cap(max_items):
    """a batch's blob area -- lay_out(): blob_cap = up256(N * 512 + 64 KB)"""
    return (512 * max_items + 65536 + 255) // 256 * 256


def _quarter(max_items):
    """the most blob bytes one call may bring -- admissible(): bb[k] > blob_cap / 4 is the call's own"""
    return _cap(max_items) // 4


Q = _quarter(8)
L17 = 17000                        # 4 L <= cap < 5 L at max_items = 8: a batch closes on blob bytes after FOUR of eight items
assert (_cap(8), Q, _quarter(64)) == (69632, 17408, 24576) and 4 * L17 <= _cap(8) < 5 * L17 and L17 <= Q


# ---- the reference: computed once per (key, message, context), shared by every test, immutable (bytes) ----
@functools.lru_cache(maxsize=None)
def _keys():
    pk, sk = orc.mldsa_keygen(PARAM, np.random.default_rng(4401).integers(0, 256, (NKEYS, 32), dtype=np.uint8))
    pk.setflags(write=False)
    sk.setflags(write=False)
    return pk, sk


@functools.lru_cache(maxsize=None)
def _msg(length, salt=0):
    return bytes(np.random.default_rng(1000003 * salt + length).integers(0, 256, length, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _ctx(length):
    return bytes((7 * i + length) & 0xFF for i in range(length))


@functools.lru_cache(maxsize=None)
def _rnd(length):
    return bytes(np.random.default_rng(77 + length).integers(0, 256, 32, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _sig(key, length, ctxlen=0, salt=0, hedged=False):
    rnd = np.frombuffer(_rnd(length), np.uint8).reshape(1, 32) if hedged else None
    return bytes(orc.mldsa_sign(PARAM, _keys()[1][key:key + 1], [_msg(length, salt)], [_ctx(ctxlen)], rnd)[0])


def _items(lens, bad=(), ctxlens=None, salt=0):
    """item i: message of lens[i] bytes under key i % NKEYS, signature bit-flipped where i is in `bad` -> idx, sig, msgs, ctxs, the oracle's verdicts"""
    n = len(lens)
    ctxlens = ctxlens or [0] * n
    idx = (np.arange(n) % NKEYS).astype(np.uint32)
    salts = [64 * salt + i if salt else 0 for i in range(n)]   # salt > 0: items of one length are still different messages
    sig = np.stack([np.frombuffer(_sig(int(idx[i]), lens[i], ctxlens[i], salts[i]), np.uint8) for i in range(n)]).copy()
    for i in bad:
        sig[i, 100 + i] ^= 1
    msgs = [_msg(lens[i], salts[i]) for i in range(n)]
    ctxs = [_ctx(c) for c in ctxlens]
    want = orc.mldsa_verify(PARAM, _keys()[0][idx], sig, msgs, ctxs)
    assert [int(w) for w in want] == [0 if i in bad else 1 for i in range(n)]   # (the fixture: a flipped bit is an invalid signature)
    return idx, sig, msgs, ctxs, want


@pytest.fixture(scope="module")
def tables():
    """tables by (kind, max_items, linger), made at first use: "plain" (the pipeline), "coalesce" (set_coalesce), "async" (a queue) over the
    public keys, "signer" (set_coalesce) over the private ones.  Tests that share one read its counters as differences."""
    from circl_amd import hostapi
    made = {}

    def get(kind, max_items=8, wait_us=0):
        key = (kind, max_items, wait_us)
        if key not in made:
            pk, sk = _keys()
            t = hostapi.KeyTable("mldsa-private" if kind == "signer" else "mldsa-public", PARAM, sk if kind == "signer" else pk)
            if kind == "async":
                t.async_start(max_items, wait_us)
            elif kind != "plain":
                t.set_coalesce(max_items, wait_us)
            made[key] = t
        return made[key]
    yield get
    for t in made.values():
        t.close()


def _sym(mult, add):
    """(mult, add) stands for a length of mult * Q + add bytes: "Q-1", "2Q+3", "0" """
    if not mult:
        return str(add)
    return ("Q" if mult == 1 else "%dQ" % mult) + ("%+d" % add if add else "")


# ---- a. blocking verify at the message limit ----
# (max_items, ((mult, add) per item: mult * Q + add bytes), items with a flipped signature bit, context bytes of item 0)
_ONE = [(1, -1), (1, 0), (1, 1), (2, 3)]
VERIFY_CASES = ([(8, (ln,), bad, 0) for ln in _ONE for bad in ((), (0,))] +
                [(8, pair, (), 0) for pair in (((1, 0), (0, 0)), ((1, -1), (0, 1)), ((1, 0), (0, 1)), ((0, 1), (1, 0)))] +
                [(8, ((1, 0),), (), 255)] +
                [(64, ((1, 0),), (), 0), (64, ((1, 1),), (0,), 0)])          # the same edge where Q = 24 576: the formula, not one point of it


def _case_id(c):
    return "N%d-%s%s%s" % (c[0], ",".join(_sym(*x) for x in c[1]), "-bad" if c[2] else "", "-ctx%d" % c[3] if c[3] else "")


@pytest.mark.parametrize("case", VERIFY_CASES, ids=_case_id)
@pytest.mark.parametrize("kind", ["coalesce", "async"])
def test_blocking_verify_at_the_message_limit(tables, kind, case):
    """The verdict is the oracle's on either side of the limit, on a coalescing table and on a table with a queue (include/circl_hip.h:
    "The blocking *_table calls keep working on such a table"), and the call joined a batch exactly when its messages are at most Q bytes."""
    max_items, lens, bad, ctxlen = case
    q = _quarter(max_items)
    lens = [m * q + a for m, a in lens]
    tab = tables(kind, max_items)
    idx, sig, msgs, ctxs, want = _items(lens, bad, [ctxlen] + [0] * (len(lens) - 1))
    before = tab.coalesce_stats()[0]
    ok = tab.verify(sig, msgs, ctxs, idx)
    joined = tab.coalesce_stats()[0] - before
    print("verify %s %s: %d message bytes, Q = %d, joined %d" % (kind, _case_id(case), sum(lens), q, joined))
    assert (ok == want).all(), (ok, want)
    assert joined == (1 if sum(lens) <= q else 0), (sum(lens), q, joined)


# ---- b. submit at the message limit ----
def test_submit_at_the_message_limit(tables):
    """*_submit has no other path: Q bytes are served, Q + 1 bytes and more than call_max items are refused at once, with nothing left behind."""
    tab = tables("async", 8)

    def submit(lens, bad=()):
        idx, sig, msgs, ctxs, want = _items(lens, bad)
        ok = np.full(len(lens), 0xAA, np.uint8)
        rc, tk = tab.submit_verify(sig, msgs, ok, ctxs=ctxs, key_idx=idx)
        done = tab.wait(tk, 5_000_000) if tk else None       # (whatever is asserted afterwards: nothing stays pending on `ok`)
        return rc, tk, ok, want, done

    for bad in ((), (0,)):
        rc, tk, ok, want, done = submit([Q], bad)
        assert rc == 0 and tk != 0 and done == 1 and (ok == want).all(), (rc, tk, done, ok, want)
    calls0, items0, _ = tab.coalesce_stats()
    rc, tk, ok, _, _ = submit([Q + 1])
    assert rc == EPARAM and tk == 0 and (ok == 0xAA).all(), (rc, tk, ok)
    rc, tk, ok, _, _ = submit([1, 2, 3])                     # more than call_max = 2 items
    assert rc == EPARAM and tk == 0 and (ok == 0xAA).all(), (rc, tk, ok)
    rc, tk, ok, _, _ = submit([Q, 1])                        # two items, one byte too many between them
    assert rc == EPARAM and tk == 0 and (ok == 0xAA).all(), (rc, tk, ok)
    rc, tk, ok, want, done = submit([90, 0], (1,))           # the next ordinary call is served as ever
    assert rc == 0 and tk != 0 and done == 1 and (ok == want).all(), (rc, tk, done, ok, want)
    calls1, items1, _ = tab.coalesce_stats()
    assert (calls1 - calls0, items1 - items0) == (1, 2)      # nothing of the refused calls entered a batch


# ---- c. batches that close on blob bytes, not on items ----
def _submit_all(tab, lens, bad, salt):
    """one-item submits of one thread, in order -> seconds the submit loop took; returns once every ticket is done and every verdict checked"""
    idx, sig, msgs, ctxs, want = _items(lens, bad, salt=salt)
    oks = [np.full(1, 0xAA, np.uint8) for _ in lens]
    tickets = []
    t0 = time.perf_counter()
    for i in range(len(lens)):
        rc, tk = tab.submit_verify(sig[i:i + 1], msgs[i:i + 1], oks[i], ctxs=ctxs[i:i + 1], key_idx=idx[i:i + 1])
        tickets.append((rc, tk))
    took = time.perf_counter() - t0
    states = [tab.wait(tk, 5_000_000) for _, tk in tickets if tk]   # (first: nothing stays pending on `oks`, whatever is asserted below)
    assert all(rc == 0 and tk != 0 for rc, tk in tickets), tickets
    assert states == [1] * len(lens), states
    got = np.concatenate(oks)
    assert (got == want).all(), (got, want)
    return took


def test_a_queue_closes_its_batches_on_blob_bytes(tables):
    """Nine 17 000-byte messages through a queue of 8-item batches that lingers 100 ms: four fill a batch's blob area, so the batches
    hold 4, 4 and 1 -- reserve() closes on bytes.  A batch that took a fifth would have written past its blob area."""
    tab = tables("async", 8, 100000)
    calls0, items0, launches0 = tab.coalesce_stats()
    took = _submit_all(tab, [L17] * 9, bad=(2, 7), salt=1)
    calls1, items1, launches1 = tab.coalesce_stats()
    calls, items, launches = calls1 - calls0, items1 - items0, launches1 - launches0
    exact = took < 0.050                                      # no batch ripens by time within half the linger
    print("queue, 9 x %d bytes: submit loop %.1f ms, calls %d, items %d, launches %d (exact branch: %s)" % (L17, took * 1e3, calls, items, launches, exact))
    assert (calls, items) == (9, 9)
    assert items <= 4 * launches, (items, launches)           # 5 L > cap: an over-admitted batch breaks this
    if exact:
        assert launches == 3, launches


MIXED = [Q, 0, 1, Q - 1, 5000, 12000, 135, 136, 137]


def test_a_queue_batches_rows_of_very_different_lengths(tables):
    """Neighbouring rows of 0 to Q bytes in shared batches, every third signature corrupt: an offset that is off by one byte anywhere
    flips a valid verdict (the message hashed is another one)."""
    tab = tables("async", 8, 100000)
    lens = MIXED * 2
    calls0, items0, launches0 = tab.coalesce_stats()
    took = _submit_all(tab, lens, bad=tuple(range(0, len(lens), 3)), salt=2)
    calls1, items1, launches1 = tab.coalesce_stats()
    calls, items, launches = calls1 - calls0, items1 - items0, launches1 - launches0
    print("queue, mixed lengths: submit loop %.1f ms, calls %d, items %d, launches %d" % (took * 1e3, calls, items, launches))
    assert (calls, items) == (len(lens), len(lens))
    assert launches < len(lens) or took >= 0.050              # (rows did share batches, unless the submitter itself was held up)


@pytest.mark.parametrize("wait_us", [0, 2000])
def test_blocking_callers_close_their_batches_on_blob_bytes(tables, wait_us):
    """Six threads, six one-item calls each, 17 000-byte messages through set_coalesce(8): every call joins (L <= Q), no batch holds
    more than four.  Without a linger a leader flushes as soon as the device has room and few batches get that far; with 2 ms of it
    the six callers of a round meet in one open batch, whose fifth caller finds it crowded."""
    tab = tables("coalesce", 8, wait_us)
    pool = 12
    idx, sig, msgs, ctxs, want = _items([L17] * pool, bad=(1, 4, 9), salt=3)
    calls0, items0, launches0 = tab.coalesce_stats()
    errs = []
    gate = threading.Barrier(6)

    def body(t):
        try:
            gate.wait()
            for k in range(6):
                i = (5 * t + 7 * k) % pool
                ok = tab.verify(sig[i:i + 1], msgs[i:i + 1], ctxs[i:i + 1], idx[i:i + 1])
                assert ok[0] == want[i], (t, k, i, ok[0], want[i])
        except Exception as e:  # noqa: BLE001 -- reported below, with the thread's number
            errs.append((t, repr(e)))
    th = [threading.Thread(target=body, args=(t,)) for t in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs[:3]
    calls1, items1, launches1 = tab.coalesce_stats()
    calls, items, launches = calls1 - calls0, items1 - items0, launches1 - launches0
    print("blocking, linger %d us, 36 x %d bytes: calls %d, items %d, launches %d" % (wait_us, L17, calls, items, launches))
    assert (calls, items) == (36, 36)
    assert items <= 4 * launches, (items, launches)


# ---- d. signing through a coalesced private table at the limit ----
SIGN_CASES = [((ln,), hedged, ctxlen) for ln in _ONE for hedged in (False, True) for ctxlen in (0, 255)] + [(((1, 0), (0, 1)), False, 0)]


def _sign_id(c):
    return "%s-%s-ctx%d" % (",".join(_sym(*x) for x in c[0]), "hedged" if c[1] else "det", c[2])


@pytest.mark.parametrize("case", SIGN_CASES, ids=_sign_id)
def test_signing_through_a_coalesced_private_table_at_the_limit(tables, case):
    """The signature is the oracle's byte for byte whether the call joined a batch (absent rnd: rows of zeros) or fell back to the
    pipeline (absent rnd: ONE row of zeros for the call, `piped_absent`); the two-item call without rnd is the fall-back's zero row."""
    lens, hedged, ctxlen = case
    lens = [m * Q + a for m, a in lens]
    n = len(lens)
    tab = tables("signer", 8)
    idx = (np.arange(n) % NKEYS).astype(np.uint32)
    msgs, ctxs = [_msg(x) for x in lens], [_ctx(ctxlen)] * n
    want = np.stack([np.frombuffer(_sig(int(idx[i]), lens[i], ctxlen, 0, hedged), np.uint8) for i in range(n)])
    rnd = np.stack([np.frombuffer(_rnd(x), np.uint8) for x in lens]) if hedged else None
    before = tab.coalesce_stats()[0]
    got = tab.sign(msgs, ctxs, rnd, idx)
    joined = tab.coalesce_stats()[0] - before
    print("sign %s: %d message bytes, joined %d" % (_sign_id(case), sum(lens), joined))
    assert (got == want).all(), np.flatnonzero((got != want).any(axis=1))
    assert joined == (1 if sum(lens) <= Q else 0), (sum(lens), joined)


# ---- e. offsets that do not start at zero ----
# the calls are items [lo, lo + n) for lo in (1, 5, 10), n in (1, 2): every one of them holds a VALID signature over a non-empty message
# with a non-empty context (a call of empty or rejected items only would pass with any offsets), next to an empty or a corrupt neighbour
POOL_LENS = [5000, 2049, 0, 135, 136, 137, 2048, 2047, 0, 1, 1, 5000]
POOL_CTXS = [3, 7, 255, 17, 1, 100, 0, 5, 255, 0, 9, 200]
POOL_BAD = (2, 3, 8)


def _shared(rows):
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.frombuffer(b"".join(rows) + bytes(16), np.uint8).copy(), off


@functools.lru_cache(maxsize=None)
def _pool():
    n = len(POOL_LENS)
    idx, sig, msgs, ctxs, want = _items(POOL_LENS, bad=POOL_BAD, ctxlens=POOL_CTXS, salt=4)
    rnd = np.random.default_rng(5).integers(0, 256, (n, 32), dtype=np.uint8)
    sk = _keys()[1][idx]
    signed = {False: orc.mldsa_sign(PARAM, sk, msgs, ctxs), True: orc.mldsa_sign(PARAM, sk, msgs, ctxs, rnd)}
    return idx, sig, _shared(msgs), _shared(ctxs), want, rnd, signed


def _at(a, i):
    return C.c_void_p(a.ctypes.data + i * a.strides[0])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("lo", [1, 5, 10])
@pytest.mark.parametrize("path", ["plain", "coalesce", "async", "submit", "sign"])
def test_offsets_that_do_not_start_at_zero(tables, path, lo, n):
    """One message blob and one context blob shared by twelve items; a call of items [lo, lo + n) passes the blobs as they are and
    &off[lo]: off[0] of the call is not 0 (copy_in's rebasing line, run_pipeline's at())."""
    from circl_amd import hostapi
    L = hostapi.nat.lib()
    idx, sig, (mb, mo), (cb, co), want, rnd, signed = _pool()
    assert mo[lo] > 0 and co[lo] > 0
    blobs = (C.c_void_p(mb.ctypes.data), _at(mo, lo), C.c_void_p(cb.ctypes.data), _at(co, lo))
    if path == "sign":
        hedged = lo != 1
        out = np.full((n, SIG), 0xAA, np.uint8)
        rc = L.circl_hip_mldsa_sign_table_keyed(tables("signer", 8).handle, _at(idx, lo), *blobs, _at(rnd, lo) if hedged else None, hostapi._p(out), n)
        assert rc == 0, rc
        assert (out == signed[hedged][lo:lo + n]).all()
        return
    ok = np.full(n, 0xAA, np.uint8)
    if path == "submit":
        tab = tables("async", 8)
        tk = C.c_uint64()
        rc = L.circl_hip_mldsa_verify_table_submit(tab.handle, _at(idx, lo), _at(sig, lo), *blobs, hostapi._p(ok), n, C.byref(tk))
        assert rc == 0 and tk.value != 0, rc
        assert tab.wait(tk.value, 5_000_000) == 1
    else:
        rc = L.circl_hip_mldsa_verify_table(tables(path, 8).handle, _at(idx, lo), _at(sig, lo), *blobs, hostapi._p(ok), n)
        assert rc == 0, rc
    assert (ok == want[lo:lo + n]).all(), (ok, want[lo:lo + n])


# ---- f. process-wide coalescing with a long message ----
def test_process_wide_coalescing_takes_long_messages_out_of_the_batch():
    """circl_hip_set_coalesce(8, 0): four threads verify one item per call with their own keys, messages of 100, Q, Q + 1 and 2Q + 3
    bytes side by side -- the long ones run on their own, the others share batches; every verdict is the oracle's.  In a process of its
    own (the switch is process-wide)."""
    code = r"""
import threading
import numpy as np
from circl_amd import hostapi, _native as nat
from oracle import orc
Q = %d
assert nat.lib().circl_hip_set_coalesce(8, 0) == 0
rng = np.random.default_rng(12)
lens = [100, Q, Q + 1, 2 * Q + 3]
pk, sk = orc.mldsa_keygen(44, rng.integers(0, 256, (4, 32), dtype=np.uint8))
msgs = [bytes(rng.integers(0, 256, x, dtype=np.uint8)) for x in lens]
good = orc.mldsa_sign(44, sk, msgs, [b""] * 4)
bad = good.copy(); bad[:, 200] ^= 8
assert orc.mldsa_verify(44, pk, good, msgs).all() and not orc.mldsa_verify(44, pk, bad, msgs).any()
errs = []
gate = threading.Barrier(4)
def body(t):
    try:
        gate.wait()
        for k in range(8):
            i, flip = (t + k) %% 4, k >= 4
            ok = hostapi.mldsa_verify(44, pk[i:i + 1], (bad if flip else good)[i:i + 1], msgs[i:i + 1])
            assert ok[0] == (0 if flip else 1), (t, k, lens[i], ok[0])
    except Exception as e:
        errs.append((t, repr(e)))
th = [threading.Thread(target=body, args=(t,)) for t in range(4)]
[x.start() for x in th]; [x.join() for x in th]
assert not errs, errs[:3]
assert nat.lib().circl_hip_set_coalesce(0, 0) == 0
print("ok")
""" % Q
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
