"""Matrix seeds that put a stream of the ML-KEM rejection sampler on the edges of the FIFO flush schedule of
circl_amd/csrc/mlkem_kernels.h (parse_shake128_block_fifo: a block of 112 candidates is checked for a flush after candidates 32, 64, 96
and 112; a fourth block only for the 0.83 % of the streams that three blocks leave short).  Found on the CPU with a model of the sampler
over hashlib.shake_128(rho || x || y): nothing here knows the kernels.  Shared by tests/test_kem_flush_inputs.py (CPU: the search finds
every shape, the model is the oracle's sampler) and tests/test_gpu_kem_flush.py / tests/kem_flush_worker.py (GPU).

A shape is a predicate over the K x K streams of one rho.  Candidates are counted from 1 over the whole stream: block 3 is candidates
225 .. 336, its checks come after candidates 256, 288, 320 and 336.

The 256th accept ON candidate 32 of block 3 (candidate 256 of the stream) or one after it needs every one (all but one) of the first
256 candidates below q: probability (3329 / 4096)^256 = 9e-24 per stream, 3e-21 for 257.  No search finds such a rho, so those two of the
positions are not among the shapes; that check is covered by the streams whose pending entries reach 32 exactly there ("pending_32_at_256":
224 accepts in the first 256 candidates, the flush at equality) or one candidate later ("pending_32_at_257": no flush at the check with
31 pending)."""
import hashlib

import numpy as np

KQ = 3329
PARAM_K = {512: 2, 768: 3, 1024: 4}
MAX_TRIES = 1 << 22


def accepts(rho, x, y, blocks=5):
    """-> bool per candidate of the first `blocks` SHAKE128 blocks of XOF(rho || x || y): candidate < q (sample.go:192-236)"""
    b = np.frombuffer(hashlib.shake_128(bytes(rho) + bytes([x, y])).digest(168 * blocks), np.uint8).astype(np.uint16).reshape(-1, 3)
    t = np.empty(2 * len(b), np.uint16)
    t[0::2] = (b[:, 0] | (b[:, 1] << 8)) & 0xFFF
    t[1::2] = (b[:, 1] >> 4) | (b[:, 2] << 4)
    return t < KQ


def sample(rho, x, y):
    """the model's polynomial: the first 256 accepted candidates"""
    b = np.frombuffer(hashlib.shake_128(bytes(rho) + bytes([x, y])).digest(168 * 5), np.uint8).astype(np.uint16).reshape(-1, 3)
    t = np.empty(2 * len(b), np.uint16)
    t[0::2] = (b[:, 0] | (b[:, 1] << 8)) & 0xFFF
    t[1::2] = (b[:, 1] >> 4) | (b[:, 2] << 4)
    return t[t < KQ][:256].astype(np.int16)


def stream_profile(rho, x, y):
    """-> (candidate at which the 256th coefficient is accepted, accepts among the first 256 candidates, among the first 257, among
    the 336 of three blocks)"""
    cum = np.cumsum(accepts(rho, x, y))
    assert cum[-1] >= 256
    return int(np.searchsorted(cum, 256)) + 1, int(cum[255]), int(cum[256]), int(cum[335])


def profile(rho, K):
    return {(x, y): stream_profile(rho, x, y) for x in range(K) for y in range(K)}


def _finish(c):
    return lambda P, K: any(p[0] == c for p in P.values())


def _stragglers(P):
    return [xy for xy, p in P.items() if p[3] < 256]


# every shape of a parameter set, in the order the batches place them
SHAPES = {
    # the 256th accept on a check of block 3 (candidates 64, 96, 112 of the block) and one candidate after each; 336 is also the very
    # last candidate of block 3, 337 the first of a fourth block
    "finish_288": _finish(288), "finish_289": _finish(289), "finish_320": _finish(320), "finish_321": _finish(321),
    "finish_336": _finish(336), "finish_337": _finish(337),
    # the check after candidate 32 of block 3 (see the module docstring)
    "pending_32_at_256": lambda P, K: any(p[1] == 224 for p in P.values()),
    "pending_32_at_257": lambda P, K: any(p[1] == 223 and p[2] == 224 for p in P.values()),
    # fourth-block stragglers: short by exactly one coefficient, short by nine or more (two chunks of the 8-entry mini FIFO), two in one
    # key, one on the first and one on the last stream of its item
    "short_by_1": lambda P, K: any(p[3] == 255 for p in P.values()),
    "short_by_9_or_more": lambda P, K: any(p[3] <= 247 for p in P.values()),
    "two_stragglers": lambda P, K: len(_stragglers(P)) >= 2,
    "straggler_first_stream": lambda P, K: _stragglers(P) == [(0, 0)],
    "straggler_last_stream": lambda P, K: _stragglers(P) == [(K - 1, K - 1)],
}


def mlkem_rho(K, d):
    """rho of the ML-KEM key made from d: the first half of SHA3-512(d || K) (cpapke.go / FIPS 203 algorithm 13)"""
    return hashlib.sha3_512(bytes(d) + bytes([K])).digest()[:32]


def search(K, seeded):
    """-> {shape: 32 bytes}: for every shape the first rho (seeded = False: rho_k = SHA3-256("kem flush rho <k>"), for an encapsulation
    key's last 32 bytes) or keygen seed d (seeded = True: d_k = SHA3-256("kem flush d <K> <k>"), rho = mlkem_rho(K, d_k)) that has it.
    Fails when a shape is not found within MAX_TRIES."""
    found, k = {}, 0
    while len(found) < len(SHAPES):
        assert k < MAX_TRIES, "no input within %d tries for %s" % (MAX_TRIES, sorted(set(SHAPES) - set(found)))
        if seeded:
            v = hashlib.sha3_256(b"kem flush d %d %d" % (K, k)).digest()
            rho = mlkem_rho(K, v)
        else:
            v = rho = hashlib.sha3_256(b"kem flush rho %d" % k).digest()
        k += 1
        P = profile(rho, K)
        for name, pred in SHAPES.items():
            if name not in found and pred(P, K):
                found[name] = v
    return {name: found[name] for name in SHAPES}


def ordinary(K, n, tag):
    """n keygen seeds d none of whose streams needs a fourth block, so that a batch has stragglers only where they are placed"""
    out, k = [], 0
    while len(out) < n:
        d = hashlib.sha3_256(b"kem flush ordinary %d %d %d" % (K, tag, k)).digest()
        k += 1
        if not _stragglers(profile(mlkem_rho(K, d), K)):
            out.append(d)
    return out


def batch_sizes(K):
    G = 64 // (K * K)  # items per workgroup of the big-batch kernels (Geom<K>::G)
    return G, (1, G - 1, G, G + 1, 2 * G + 3)


def placements(K, nshapes):
    """-> [(n, {position: shape index})]: every batch size with the shapes, a few at a time, in its first item, its last item (next to the
    padding lanes of a partial group), and the items on both sides of the first group's end; then one group whose first item has its straggler
    on lane 0 and whose last item has it on the group's last active lane (two parked streams, adopted by rank)."""
    G, sizes = batch_sizes(K)
    out = []
    for n in sizes:
        pos = sorted({p for p in (0, G - 1, G, n - 1) if 0 <= p < n})
        for s0 in range(0, nshapes, len(pos)):
            out.append((n, {p: s for p, s in zip(pos, range(s0, nshapes))}))
    names = list(SHAPES)
    out.append((G, {0: names.index("straggler_first_stream"), G - 1: names.index("straggler_last_stream")}))
    return out
