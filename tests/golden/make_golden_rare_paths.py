"""Generates tests/golden/rare_paths.json.gz: inputs that take the sampler and rejection-loop paths random material almost never
takes (tests/test_oracle_rare_paths.py proves every property claimed here; tests/test_gpu_rare_paths.py and
tests/test_gpu_mldsa_extremes.py run the HIP kernels on them).

Deterministic: increasing integer seeds (32-byte little-endian) through hashlib, and for `sign_rejections` the oracle's signing trace
(orc.mldsa_sign_trace).  Only data is written: seeds, rhos, messages, observed counts and traces.

    python tests/golden/make_golden_rare_paths.py
"""
import gzip
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from oracle import orc  # noqa: E402
from rare_inputs import DSA, accepted_in_3_blocks, accepted_nibbles, dsa_rhoprime, kem_rho, sk_with_t0_bytes  # noqa: E402


def le32(i):
    return int(i).to_bytes(32, "little")


# ---- ML-DSA secret polynomials: SHAKE256(rho' || LE16(nonce)), nibbles accepted when <= 8 (eta 4) / <= 14 (eta 2) --------------------
def find_eta4_third_block(param, want=4):
    """keygen seeds with a secret polynomial that accepts fewer than 256 of the 544 nibbles of two blocks; at least `want`, and on until
    an s1 polynomial (nonce < L) and an s2 polynomial are both among them"""
    K, L = DSA[param][:2]
    hits, seed = [], 0
    while len(hits) < want or not any(n < L for h in hits for n in h["nonces"]) or not any(n >= L for h in hits for n in h["nonces"]):
        rp = dsa_rhoprime(param, le32(seed))
        cnt = [accepted_nibbles(param, rp, n, 2) for n in range(K + L)]
        short = [n for n in range(K + L) if cnt[n] < 256]
        if short:
            hits.append({"seed": seed, "xi": le32(seed).hex(), "nonces": short, "accepted_in_544": [cnt[n] for n in short]})
        seed += 1
    return hits, seed


def find_eta2_block1(param):
    """the first seeds whose polynomial `nonce` (0, L and K + L - 1 in turn) accepts >= 257 / exactly 256 / exactly 255 of block 1's 272 nibbles"""
    K, L = DSA[param][:2]
    out = {"inside_block1": [], "exactly_256": [], "exactly_255": []}
    searched = 0
    for nonce in (0, L, K + L - 1):
        need = {"inside_block1": lambda c: c >= 257, "exactly_256": lambda c: c == 256, "exactly_255": lambda c: c == 255}
        seed = 0
        while need:
            c = accepted_nibbles(param, dsa_rhoprime(param, le32(seed)), nonce, 1)
            for k in [k for k, f in need.items() if f(c)]:
                out[k].append({"seed": seed, "xi": le32(seed).hex(), "nonce": nonce, "accepted_in_272": c})
                del need[k]
            seed += 1
        searched = max(searched, seed)
    return out, searched


# ---- ML-KEM / Kyber matrix streams: SHAKE128(rho || x || y), 12-bit candidates accepted when < q; three blocks hold 336 ----------------
def find_kem(scheme, K):
    """per stream (x, y) a key whose stream needs a fourth block, a key with two such streams, and the two boundaries"""
    z = hashlib.sha3_256(b"rare paths z").digest()
    want = {"multi": None, "exactly_256": None, "exactly_255": None}
    want.update({(x, y): None for x in range(K) for y in range(K)})
    d = 0
    while any(v is None for v in want.values()):
        rho = kem_rho(scheme, K, le32(d))
        cnt = {(x, y): accepted_in_3_blocks(rho, x, y) for x in range(K) for y in range(K)}
        fourth = [list(xy) for xy, c in cnt.items() if c < 256]
        rec = {"d": d, "seed": (le32(d) + z).hex(), "rho": rho.hex(), "fourth": fourth}
        for x, y in fourth:
            if want[(x, y)] is None:
                want[(x, y)] = dict(rec, xy=[x, y])
        if len(fourth) >= 2 and want["multi"] is None:
            want["multi"] = rec
        for c, k in ((256, "exactly_256"), (255, "exactly_255")):
            at = [list(xy) for xy, v in cnt.items() if v == c]
            if at and want[k] is None:
                want[k] = dict(rec, xy=at[0], accepted_in_336=c)
        d += 1
    return {"positions": [want[(x, y)] for x in range(K) for y in range(K)], "multi": want["multi"], "exactly_256": want["exactly_256"],
            "exactly_255": want["exactly_255"]}, d


# ---- signing: messages chosen with the oracle's trace ----------------------------------------------------------------------------------
# causes: 1 |w0 - c s2|, 2 |z|, 3 |c t0|, 4 hint weight (orc.SIGN_CAUSES).  With a key that KeyGen made, cause 3 cannot be searched for:
# |t0| <= 2^12 and c has tau coefficients +-1, so |c t0| <= tau 2^12 = 200 704 (tau 49) / 245 760 (tau 60) < gamma2 = 261 888 for
# ML-DSA-65 / -87 and Dilithium3 / 5 -- the check never fires --, and for ML-DSA-44 / Dilithium2 (gamma2 = 95 232, tau 39) a coefficient
# of c t0 is a sum of 39 terms uniform in +-2^12 (sigma 14 800): 6.4 sigma, about 1e-7 per attempt.  The private key's t0 is the
# caller's, though: the same key with every t0 coefficient 2^12 (the 416-byte field all 0x00) or -2^12 + 1 (all 0xFF) makes
# c t0 = 2^12 * (signed sums of c), which passes gamma2 in a few per cent of the attempts at tau 39.  `t0_saturated` holds such items.
def find_sign_rejections(param, pool):
    """One key; messages b"rare-paths message <k>" in increasing k.  `items`: the first message signed at the first attempt, the first
    three with 20..199 attempts, and then the first ones that add a rejection by hint weight until causes 1, 2 and 4 have each been seen
    three times.  `t0_saturated`: per t0 filling the first message signed at once and the first of 20..199 attempts, and for tau = 39 the
    first ones that add a rejection by |c t0| until there are three.  A message the oracle needs 200 or more attempts for is never kept."""
    xi = hashlib.sha3_256(b"rare paths signing key %d" % param).digest()
    _, sk = orc.mldsa_keygen(param, np.frombuffer(xi, np.uint8))
    sk = sk[0].tobytes()
    stats = {}

    def search(key, need_causes, nlong, extra):
        items, seen, longs, first, k = [], {1: 0, 2: 0, 3: 0, 4: 0}, 0, False, 0
        done = lambda: first and longs >= nlong and all(seen[c] >= 3 for c in need_causes)
        while not done():
            msgs = [b"rare-paths message %d" % i for i in range(k, k + 256)]
            for msg, tr in zip(msgs, pool.map(lambda m: orc.mldsa_sign_trace(param, key, m), msgs)):
                k += 1
                if tr is None or tr[1] >= 200:
                    continue
                _, att, causes = tr
                if not ((att == 1 and not first) or (att >= 20 and longs < nlong) or any(seen[c] < 3 and c in causes for c in need_causes if c >= 3)):
                    continue
                first |= att == 1
                longs += att >= 20
                for c in causes:
                    seen[c] += 1
                items.append(dict(extra, msg=msg.hex(), attempts=att, causes=causes))
                if done():
                    break
        return items, k

    out = {"xi": xi.hex()}
    out["items"], k = search(sk, (1, 2, 4), 3, {})
    stats["messages_searched"] = k
    out["t0_saturated"] = []
    for byte in (0x00, 0xFF):
        got, k = search(sk_with_t0_bytes(param, sk, byte), (3,) if DSA[param][2] == 2 and DSA[param][0] == 4 else (), 1, {"t0_byte": byte})
        out["t0_saturated"] += got
        stats["messages_searched_t0_%02x" % byte] = k
    for name in ("items", "t0_saturated"):
        stats[name] = {"count": len(out[name]), "longest_chain": max(i["attempts"] for i in out[name]),
                       "items_per_cause": {orc.SIGN_CAUSES[c]: sum(c in i["causes"] for i in out[name]) for c in (1, 2, 3, 4)},
                       "rejections_per_cause": {orc.SIGN_CAUSES[c]: sum(i["causes"].count(c) for i in out[name]) for c in (1, 2, 3, 4)}}
    return out, stats


def main():
    out = {"eta4_third_block": {}, "eta2_second_block": {}, "kem_fourth_block": {"mlkem": {}, "kyber": {}}, "sign_rejections": {}, "searched": {}}
    for param in (65, 3):
        out["eta4_third_block"][str(param)], n = find_eta4_third_block(param)
        out["searched"]["eta4_third_block/%d" % param] = {"seeds_searched": n, "hits": len(out["eta4_third_block"][str(param)])}
    for param in (44, 87):
        out["eta2_second_block"][str(param)], n = find_eta2_block1(param)
        out["searched"]["eta2_second_block/%d" % param] = {"seeds_searched": n}
    for scheme in ("mlkem", "kyber"):
        for K in (2, 3, 4):
            out["kem_fourth_block"][scheme][str(K)], n = find_kem(scheme, K)
            out["searched"]["kem_fourth_block/%s/%d" % (scheme, K)] = {"seeds_searched": n}
    with ThreadPoolExecutor(orc.ncpu()) as pool:
        for param in (44, 65, 87, 2, 3, 5):
            out["sign_rejections"][str(param)], out["searched"]["sign_rejections/%d" % param] = find_sign_rejections(param, pool)
    path = os.path.join(HERE, "rare_paths.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode())
    print(json.dumps(out["searched"], indent=1))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
