"""Batch Ed448 (sign/ed448: NewKeyFromSeed, Sign, Verify with a context) on the GPU through the C ABI, against the reference's
own vectors (tests/golden/curve448.json.gz: Wycheproof, which contains the RFC 8032 7.4 vectors) and the RFC 8032 5.2 checker
of tests/curve448.py."""
import ctypes as C

import numpy as np
import pytest

import curve448 as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
P, L = ref.P, ref.L


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


def _rows(hexes, width):
    return np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), np.uint8).reshape(-1, width).copy()


def test_fixture_keygen_resign_and_verdicts(api):
    G = load_golden("curve448.json.gz")["wycheproof"]
    assert len(G) == 86
    keys = sorted({(v["sk"], v["pk"]) for v in G})
    assert len(keys) == 9
    pk, sk = api.ed448_keygen(_rows((k[0] for k in keys), 57))
    assert [bytes(r).hex() for r in pk] == [k[1] for k in keys]
    assert [bytes(r).hex() for r in sk] == [k[0] + k[1] for k in keys]
    V = [v for v in G if v["valid"]]
    assert len(V) == 17
    _, sk = api.ed448_keygen(_rows((v["sk"] for v in V), 57))
    sig = api.ed448_sign(sk, [bytes.fromhex(v["msg"]) for v in V])  # the empty context, as wycheproof_test.go signs
    assert [bytes(r).hex() for r in sig] == [v["sig"] for v in V]
    ok = api.ed448_verify([bytes.fromhex(v["pk"]) for v in G], [bytes.fromhex(v["sig"]) for v in G], [bytes.fromhex(v["msg"]) for v in G])
    assert [bool(x) for x in ok] == [v["valid"] for v in G], [v["tcId"] for v, x in zip(G, ok) if bool(x) != v["valid"]]


def _ragged_cases(rng):
    """(context length, message length): every message length 0..300, and the lengths that put the end of dom4 || prefix || M
    (10 + c + 57 + m) and of dom4 || R || A || M (10 + c + 114 + m) one before, on and one after a 136-byte block boundary"""
    cases = []
    ctx_cycle = [0, 1, 255, None]
    for m in range(301):
        c = ctx_cycle[m % 4]
        cases.append((int(rng.integers(2, 255)) if c is None else c, m))
    for c in (0, 1, 255, int(rng.integers(2, 255))):
        for head in (10 + c + 57, 10 + c + 114):
            for blocks in range(1, 10):
                for d in (-1, 0, 1):
                    m = blocks * 136 - head + d
                    if 0 <= m <= 1100:
                        cases.append((c, m))
    cases += [(0, 1100), (255, 1100), (1, 1099)]
    cases += [(int(rng.integers(0, 256)), int(rng.integers(301, 1101))) for _ in range(96)]
    return cases


def test_ragged_batch_with_contexts(api):
    rng = np.random.default_rng(21)
    cases = _ragged_cases(rng)
    n = len(cases)
    assert n >= 512 and {m for _, m in cases} >= set(range(301)) and max(m for _, m in cases) == 1100
    pk, sk = api.ed448_keygen(rng.integers(0, 256, (n, 57), dtype=np.uint8))
    ctxs = [rng.bytes(c) for c, _ in cases]
    msgs = [rng.bytes(m) for _, m in cases]
    sig = api.ed448_sign(sk, msgs, ctxs)
    for i in range(0, n, 4):
        assert bytes(sig[i]) == ref.sign(bytes(sk[i]), msgs[i], ctxs[i]), cases[i]
    assert api.ed448_verify(pk, sig, msgs, ctxs).all()
    other_ctx = [bytes([c[0] ^ 1]) + c[1:] if c else b"x" for c in ctxs]
    assert not api.ed448_verify(pk, sig, msgs, other_ctx).any()
    other_msg = [bytes([m[0] ^ 1]) + m[1:] if m else b"\1" for m in msgs]
    assert not api.ed448_verify(pk, sig, other_msg, ctxs).any()
    for col, what in ((3, "R"), (57 + 9, "S")):
        bad = sig.copy()
        bad[:, col] ^= 0x10
        assert not api.ed448_verify(pk, bad, msgs, ctxs).any(), what
    badk = pk.copy()
    badk[:, 11] ^= 0x04
    assert not api.ed448_verify(badk, sig, msgs, ctxs).any()
    # ctxs=None is the empty context for every item
    e = [i for i, (c, _) in enumerate(cases) if c == 0]
    assert api.ed448_verify(pk[e], sig[e], [msgs[i] for i in e]).all()
    assert (api.ed448_sign(sk[e], [msgs[i] for i in e]) == sig[e]).all()


def test_rejects(api):
    from circl_amd import _native as nat
    rng = np.random.default_rng(22)
    seed = rng.bytes(57)
    pk = ref.public(seed)
    msg, ctx = b"rejects", b"ctx"
    sig = ref.sign(seed + pk, msg, ctx)
    S = int.from_bytes(sig[57:], "little")
    assert S + L < 2**448
    e = lambda y, top=0: y.to_bytes(56, "little") + bytes([top])  # noqa: E731
    cases = [(pk, sig[:57] + (S + L).to_bytes(57, "little"), ctx),          # S + l fits in 56 bytes
             (pk, sig[:113] + b"\x01", ctx)]                                # byte 56 of S
    cases += [(pk[:56] + bytes([pk[56] | 1 << b]), sig, ctx) for b in range(7)]  # the low seven bits of byte 56 of the key
    cases += [(e(P), sig, ctx), (e(P + 1), sig, ctx), (e(1, 0x80), sig, ctx), (e(ref.y_without_x()), sig, ctx)]
    cases += [(pk, sig, bytes(256))]
    ok = api.ed448_verify([c[0] for c in cases], [c[1] for c in cases], [msg] * len(cases), [c[2] for c in cases])
    assert not ok.any(), [i for i, x in enumerate(ok) if x]
    assert [ref.verify(c[0], msg, c[1], c[2]) for c in cases] == [False] * len(cases)
    assert api.ed448_verify([pk], [sig], [msg], [ctx]).all()
    # wrong-length rows are false through the binding, without a launch
    ok = api.ed448_verify([pk, pk[:56], pk + b"\0", pk], [sig, sig, sig, sig[:113]], [msg] * 4, [ctx] * 4)
    assert [int(x) for x in ok] == [1, 0, 0, 0]
    # signing with a context over 255 bytes is refused before any launch
    with pytest.raises(nat.CirclHipError):
        api.ed448_sign(np.frombuffer(seed + pk, np.uint8).reshape(1, 114), [msg], [bytes(256)])


def test_verification_rule_is_the_references(api):
    """The reference verifies enc(CombinedMult(S, k, -A)) == R, and goldilocks.Curve.CombinedMult (ecc/goldilocks/curve.go:80-90)
    divides both scalars by 4 mod l, maps to the 4-isogenous twist and back -- a multiplication by 4 -- so the result is
    [S]B - [k]A0 with A0 = A without its 4-torsion component.  Expected verdicts: (a) a key carrying a torsion component with a
    signature made for those key bytes is ACCEPTED (cofactorless verification refuses some of them); (b) an R carrying a torsion
    component is REFUSED (cofactored verification accepts them all); (c) the identity as key, R = enc([S]B): accepted.  The
    reference cannot be run where this project is built (no Go toolchain): these expectations rest on reading curve.go and
    isogeny.go, whose formulas have no exceptional case on the four 4-torsion points.  The Wycheproof vectors do not separate
    the three rules (all three give the reference's verdict on all 86), so the constructed cases are what pins the rule."""
    rng = np.random.default_rng(23)
    nkeys = 24
    pks, sigs, msgs, want, kind = [], [], [], [], []
    for t_name, T in (("order4", ref.T4), ("order2", ref.T2)):
        for j in range(nkeys):
            seed, msg = rng.bytes(57), rng.bytes(int(rng.integers(0, 80)))
            honest = ref.public(seed)
            A0 = ref.decode(honest)
            # (a) public key enc(A0 + T), signed for those bytes (k is hashed over them)
            pk_t = ref.encode(ref.add(A0, T))
            pks.append(pk_t), sigs.append(ref.sign(seed + pk_t, msg)), msgs.append(msg), want.append(1), kind.append(("a", t_name))
            # (b) honest key, R' = enc([r]B + T), S = r + k' s with k' hashed over R'
            r, _, s, _ = ref.sign_parts(seed + honest, msg)
            R_t = ref.encode(ref.add(ref.mul(r, ref.B), T))
            S = (r + ref.challenge(R_t, honest, msg) * s) % L
            pks.append(honest), sigs.append(R_t + S.to_bytes(57, "little")), msgs.append(msg), want.append(0), kind.append(("b", t_name))
            # (c) the identity as public key: any message, R = enc([S]B)
            S = int.from_bytes(rng.bytes(64), "little") % L
            pks.append(ref.encode(ref.IDENTITY)), sigs.append(ref.base_mult(S) + S.to_bytes(57, "little")), msgs.append(msg), want.append(1)
            kind.append(("c", t_name))
    assert [ref.verify(p, m, s) for p, m, s in zip(pks, msgs, sigs)] == [bool(w) for w in want]
    # the cases separate the rules: otherwise this test proves nothing
    a_cofactorless = [ref.verify(p, m, s, rule="cofactorless") for p, m, s, k in zip(pks, msgs, sigs, kind) if k[0] == "a"]
    b_cofactored = [ref.verify(p, m, s, rule="cofactored") for p, m, s, k in zip(pks, msgs, sigs, kind) if k[0] == "b"]
    assert not all(a_cofactorless) and all(b_cofactored)
    ok = api.ed448_verify(pks, sigs, msgs)
    assert [int(x) for x in ok] == want, [k for k, x, w in zip(kind, ok, want) if int(x) != w]


def test_large_batch_every_device_and_all_devices(api):
    rng = np.random.default_rng(24)
    n = 1 << 16
    seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
    pk, sk = api.ed448_keygen(seeds, device=-1)
    msgs = [bytes(r) for r in rng.integers(0, 256, (n, 64), dtype=np.uint8)]
    sig = api.ed448_sign(sk, msgs, device=-1)
    for i in rng.choice(n, 256, replace=False):
        assert bytes(pk[i]) == ref.public(bytes(seeds[i])), i
        assert bytes(sig[i]) == ref.sign(bytes(sk[i]), msgs[i]), i
    assert api.ed448_verify(pk, sig, msgs, device=-1).all()
    bad = sig.copy()
    bad[::3, 5] ^= 4
    ok = api.ed448_verify(pk, bad, msgs, device=-1)
    assert (ok[::3] == 0).all() and (np.delete(ok, np.s_[::3]) == 1).all()
    m = 3000
    for d in range(api.device_count()):
        p2, s2 = api.ed448_keygen(seeds[:m], device=d)
        assert (p2 == pk[:m]).all() and (s2 == sk[:m]).all(), d
        assert (api.ed448_sign(sk[:m], msgs[:m], device=d) == sig[:m]).all(), d
        assert api.ed448_verify(pk[:m], sig[:m], msgs[:m], device=d).all(), d


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_batch_sizes(api, n):
    rng = np.random.default_rng(n)
    seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
    pk, sk = api.ed448_keygen(seeds)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 200, n)]
    ctxs = [rng.bytes(int(l)) for l in rng.integers(0, 40, n)]
    sig = api.ed448_sign(sk, msgs, ctxs)
    for i in sorted({0, n // 2, n - 1}) if n else []:
        assert bytes(pk[i]) == ref.public(bytes(seeds[i]))
        assert bytes(sig[i]) == ref.sign(bytes(sk[i]), msgs[i], ctxs[i])
    ok = api.ed448_verify(pk, sig, msgs, ctxs)
    assert ok.shape == (n,) and ok.all()


def test_foreign_public_half(api):
    rng = np.random.default_rng(25)
    pk, sk = api.ed448_keygen(rng.integers(0, 256, (4, 57), dtype=np.uint8))
    bad = sk.copy()
    bad[:, 57:] = pk[::-1]  # the public half of another key, hashed as stored
    msgs = [b"abc", b"", b"x" * 300, b"q"]
    sig = api.ed448_sign(bad, msgs)
    assert [bytes(s) for s in sig] == [ref.sign(bytes(k), m) for k, m in zip(bad, msgs)]
    good = api.ed448_sign(sk, msgs)
    assert (sig[:, :57] == good[:, :57]).all() and (sig[:, 57:] != good[:, 57:]).any(axis=1).all()


def test_dev_forms_on_a_caller_stream(api):
    import torch
    from circl_amd import _native as nat
    rng = np.random.default_rng(26)
    n = 300
    seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
    msgs = [rng.bytes(int(l)) for l in rng.integers(0, 500, n)]
    ctxs = [rng.bytes(int(l)) for l in rng.integers(0, 256, n)]
    mb, mo = api._blob(msgs)
    cb, co = api._blob(ctxs)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_seed, d_mb, d_mo, d_cb, d_co = t(seeds), t(mb), t(mo.view(np.int64)), t(cb), t(co.view(np.int64))
    d_pk = torch.empty((n, 57), dtype=torch.uint8, device=dev)
    d_sk = torch.empty((n, 114), dtype=torch.uint8, device=dev)
    d_sig = torch.empty((n, 114), dtype=torch.uint8, device=dev)
    d_sig0 = torch.empty((n, 114), dtype=torch.uint8, device=dev)
    d_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    d_ok0 = torch.empty(n, dtype=torch.uint8, device=dev)
    L_ = nat.lib()
    ws_bytes = L_.circl_hip_ed448_workspace_size(n)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    st = C.c_void_p(s.cuda_stream)
    with torch.cuda.stream(s):
        nat.check(L_.circl_hip_ed448_keygen_dev(vp(d_seed), vp(d_pk), vp(d_sk), n, vp(d_ws), ws_bytes, st), "keygen_dev")
        nat.check(L_.circl_hip_ed448_sign_dev(vp(d_sk), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_sig), n, vp(d_ws), ws_bytes, st), "sign_dev")
        nat.check(L_.circl_hip_ed448_verify_dev(vp(d_pk), vp(d_sig), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_ok), n, vp(d_ws), ws_bytes, st), "verify_dev")
        nat.check(L_.circl_hip_ed448_sign_dev(vp(d_sk), vp(d_mb), vp(d_mo), None, None, vp(d_sig0), n, None, 0, st), "sign_dev, no contexts")
        nat.check(L_.circl_hip_ed448_verify_dev(vp(d_pk), vp(d_sig0), vp(d_mb), vp(d_mo), None, None, vp(d_ok0), n, vp(d_ws), ws_bytes, st), "verify_dev")
        assert L_.circl_hip_ed448_verify_dev(vp(d_pk), vp(d_sig), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_ok), n, vp(d_ws), ws_bytes - 256, st) == nat.EWORKSPACE
    s.synchronize()
    pk, sk, sig, sig0 = d_pk.cpu().numpy(), d_sk.cpu().numpy(), d_sig.cpu().numpy(), d_sig0.cpu().numpy()
    assert d_ok.cpu().numpy().all() and d_ok0.cpu().numpy().all()
    hpk, hsk = api.ed448_keygen(seeds)
    assert (pk == hpk).all() and (sk == hsk).all()
    assert (sig == api.ed448_sign(hsk, msgs, ctxs)).all() and (sig0 == api.ed448_sign(hsk, msgs)).all()
    assert bytes(sig[7]) == ref.sign(bytes(sk[7]), msgs[7], ctxs[7]) and bytes(sig0[7]) == ref.sign(bytes(sk[7]), msgs[7])


def test_dev_forms_with_a_context_over_255_bytes(api):
    # the _dev forms cannot see the offsets before the launch: signing writes an all-zero signature for such an item (the host
    # form refuses the whole call), verification answers 0 for it; its neighbours are untouched
    import torch
    from circl_amd import _native as nat
    rng = np.random.default_rng(27)
    n = 3
    seeds = rng.integers(0, 256, (n, 57), dtype=np.uint8)
    msgs, ctxs = [b"one", b"two", b"three"], [b"", bytes(256), b"ctx-5"]
    pk, sk = api.ed448_keygen(seeds)
    mb, mo = api._blob(msgs)
    cb, co = api._blob(ctxs)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_pk, d_sk, d_mb, d_mo, d_cb, d_co = t(pk), t(sk), t(mb), t(mo.view(np.int64)), t(cb), t(co.view(np.int64))
    d_sig = torch.full((n, 114), 0xAA, dtype=torch.uint8, device=dev)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    L_ = nat.lib()
    ws_bytes = L_.circl_hip_ed448_workspace_size(n)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nat.check(L_.circl_hip_ed448_sign_dev(vp(d_sk), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_sig), n, None, 0, st), "sign_dev")
    nat.check(L_.circl_hip_ed448_verify_dev(vp(d_pk), vp(d_sig), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_ok), n, vp(d_ws), ws_bytes, st), "verify_dev")
    torch.cuda.synchronize()
    sig, ok = d_sig.cpu().numpy(), d_ok.cpu().numpy()
    assert not sig[1].any() and [int(x) for x in ok] == [1, 0, 1]
    for i in (0, 2):
        assert bytes(sig[i]) == ref.sign(bytes(sk[i]), msgs[i], ctxs[i])
    # a good signature under a context of 256 bytes is refused too
    good = t(np.frombuffer(ref.sign(bytes(sk[1]), msgs[1], b""), np.uint8).reshape(1, 114).copy())
    d_sig[1] = good[0]
    nat.check(L_.circl_hip_ed448_verify_dev(vp(d_pk), vp(d_sig), vp(d_mb), vp(d_mo), vp(d_cb), vp(d_co), vp(d_ok), n, vp(d_ws), ws_bytes, st), "verify_dev")
    torch.cuda.synchronize()
    assert [int(x) for x in d_ok.cpu().numpy()] == [1, 0, 1]
