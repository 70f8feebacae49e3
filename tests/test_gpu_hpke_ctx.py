"""HPKE contexts on the GPU -- setup of both sides, ChaCha20-Poly1305 Seal / Open, Export and the single-shot forms -- against the
RFC 9180 vectors of tests/golden/hpke_ctx.json.gz and the checker tests/hpke_ctx.py, through the host-buffer and the device-resident
forms of the C ABI."""
import numpy as np
import pytest

import hpke_ctx as hc
import hpke_dhkem as hp
from conftest import hx, load_golden

pytestmark = pytest.mark.gpu
VECTORS = load_golden("hpke_ctx.json.gz")
KEMS, KDFS = [0x20, 0x21], [1, 3]
N = 130   # two full wavefronts and a two-lane tail


@pytest.fixture(scope="module")
def api():
    from circl_amd import hostapi
    return hostapi


@pytest.fixture(scope="module")
def dev():
    import torch
    from circl_amd import device
    torch.cuda.set_device(0)
    return device


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared reference arrays are read-only)


def _seq(values):
    return _t(np.array(values, np.uint64).view(np.int64))


def _rows(items):
    return np.frombuffer(b"".join(items), np.uint8).reshape(len(items), -1).copy()


def _split(flat, lens, extra=0):
    """the items of a flat ciphertext (extra = 16) or plaintext tensor / array"""
    flat = flat.cpu().numpy() if hasattr(flat, "cpu") else flat
    off = np.concatenate([[0], np.cumsum(lens)])
    return [flat[int(off[k]) + extra * k:int(off[k + 1]) + extra * (k + 1)].tobytes() for k in range(len(lens))]


def kem_reference(kem):
    """test_gpu_hpke.py's checker run on 130 random items per KEM (keys, enc, shared secrets), computed once per session and read-only"""
    import test_gpu_hpke
    return test_gpu_hpke.reference(kem)


# ---- the RFC 9180 vectors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kem", KEMS)
def test_rfc9180_vectors(api, dev, kem):
    vs = [v for v in VECTORS if v["kem_id"] == kem]
    assert len(vs) == 16
    for v in vs:
        kdf, aead, mode = v["kdf_id"], v["aead_id"], v["mode"]
        auth, with_psk = mode in (2, 3), mode in (1, 3)
        row = lambda name: _rows([hx(v[name])])
        info = [hx(v["info"])]
        psk, psk_id = ([hx(v["psk"])], [hx(v["psk_id"])]) if with_psk else (None, None)
        skS, pkS = (row("skSm"), row("pkSm")) if auth else (None, None)
        want = hx(v["key"]).ljust(32, b"\0") + hx(v["base_nonce"]).ljust(12, b"\0") + bytes(4) + hx(v["exporter_secret"])
        h = api.HpkeSuite(kem, kdf, aead)
        d = dev.HpkeSuiteDevice(kem, kdf, aead)
        R = lambda items: None if items is None else dev.Ragged(items)
        T = lambda a: None if a is None else _t(a)

        # setup on both sides, host and device forms
        enc, ctx, ok = h.setup_sender(mode, row("pkRm"), row("ikmE"), info, psk, psk_id, skS, pkS)
        assert (enc.tobytes(), ctx.tobytes(), ok.tolist()) == (hx(v["enc"]), want, [1])
        for pkR in (None, row("pkRm")):
            ctx_r, ok = h.setup_receiver(mode, row("skRm"), enc, info, psk, psk_id, pkS, pkR)
            assert (ctx_r.tobytes(), ok.tolist()) == (want, [1])
        enc_d, ctx_d, ok_d = d.setup_sender(mode, _t(row("pkRm")), _t(row("ikmE")), R(info), R(psk), R(psk_id), T(skS), T(pkS))
        assert (enc_d.cpu().numpy().tobytes(), ctx_d.cpu().numpy().tobytes(), ok_d.tolist()) == (hx(v["enc"]), want, [1])
        ctx_d, ok_d = d.setup_receiver(mode, _t(row("skRm")), enc_d, R(info), R(psk), R(psk_id), T(pkS))
        assert (ctx_d.cpu().numpy().tobytes(), ok_d.tolist()) == (want, [1])

        # Export on context rows and single-shot
        exps, vals = [hx(x["exporter_context"]) for x in v["exports"]], _rows([hx(x["exported_value"]) for x in v["exports"]])
        ctx3 = np.repeat(ctx, 3, axis=0)
        assert (h.export(ctx3, exps, 32) == vals).all()
        assert (d.export(_t(ctx3), dev.Ragged(exps), 32).cpu().numpy() == vals).all()
        for k, e in enumerate(exps):
            enc1, out, ok = h.export_single(mode, row("pkRm"), row("ikmE"), [e], 32, info, psk, psk_id, skS, pkS)
            assert (enc1.tobytes(), out.tobytes(), ok.tolist()) == (hx(v["enc"]), vals[k].tobytes(), [1])
            out, ok = h.export_single_receiver(mode, row("skRm"), enc, [e], 32, info, psk, psk_id, pkS)
            assert (out.tobytes(), ok.tolist()) == (vals[k].tobytes(), [1])
        enc1, out, ok = d.export_single(mode, _t(row("pkRm")), _t(row("ikmE")), dev.Ragged(exps[2:]), 32, R(info), R(psk), R(psk_id), T(skS), T(pkS))
        assert (enc1.cpu().numpy().tobytes(), out.cpu().numpy().tobytes(), ok.tolist()) == (hx(v["enc"]), vals[2].tobytes(), [1])
        out, ok = d.export_single_receiver(mode, _t(row("skRm")), enc_d, dev.Ragged(exps[2:]), 32, R(info), R(psk), R(psk_id), T(pkS))
        assert (out.cpu().numpy().tobytes(), ok.tolist()) == (vals[2].tobytes(), [1])
        if aead == hc.AEAD_EXPORT_ONLY:
            continue

        # Seal / Open at the six sequence numbers as one batch, host and device forms
        es = v["encryptions"]
        seqs, pts, aads, cts = [e["seq"] for e in es], [hx(e["pt"]) for e in es], [hx(e["aad"]) for e in es], [hx(e["ct"]) for e in es]
        ctx6 = np.repeat(ctx, 6, axis=0)
        assert h.seal(ctx6, pts, aads, seqs) == cts
        got, ok = h.open(ctx6, cts, aads, seqs)
        assert got == pts and ok.all()
        lens = [len(p) for p in pts]
        ct_d = d.seal(_t(ctx6), dev.Ragged(pts), dev.Ragged(aads), _seq(seqs))
        assert _split(ct_d, lens, 16) == cts
        pt_d, ok_d = d.open(_t(ctx6), ct_d, dev.Ragged(pts), dev.Ragged(aads), _seq(seqs))
        assert _split(pt_d, lens) == pts and ok_d.cpu().numpy().all()

        # single-shot at sequence number 0
        enc1, ct1, ok = h.seal_single(mode, row("pkRm"), row("ikmE"), pts[:1], aads[:1], info, psk, psk_id, skS, pkS)
        assert (enc1.tobytes(), ct1, ok.tolist()) == (hx(v["enc"]), cts[:1], [1])
        pt1, ok = h.open_single(mode, row("skRm"), enc, cts[:1], aads[:1], info, psk, psk_id, pkS)
        assert (pt1, ok.tolist()) == (pts[:1], [1])
        enc1, ct1, ok = d.seal_single(mode, _t(row("pkRm")), _t(row("ikmE")), dev.Ragged(pts[:1]), dev.Ragged(aads[:1]), R(info), R(psk), R(psk_id), T(skS), T(pkS))
        assert (enc1.cpu().numpy().tobytes(), _split(ct1, lens[:1], 16), ok.tolist()) == (hx(v["enc"]), cts[:1], [1])
        pt1, ok = d.open_single(mode, _t(row("skRm")), enc_d, ct1, dev.Ragged(pts[:1]), dev.Ragged(aads[:1]), R(info), R(psk), R(psk_id), T(pkS))
        assert (_split(pt1, lens[:1]), ok.tolist()) == (pts[:1], [1])


# ---- one ragged batch of 130 per (kem, kdf) against the checker ----------------------------------------------------------------
def ragged_inputs():
    rng = np.random.default_rng(9180)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return dict(pt=[rnd(i) for i in range(N)], aad=[rnd(i % 41) for i in range(N)], psk=[rnd(32 + i % 40) for i in range(N)],
                psk_id=[rnd(1 + i % 30) for i in range(N)], info=[rnd(i + 20) for i in range(N)])


@pytest.mark.parametrize("kem", KEMS)
@pytest.mark.parametrize("kdf", KDFS)
def test_ragged_batch_against_the_checker(api, dev, kem, kdf):
    k, r, s = kem_reference(kem), ragged_inputs(), hc.Suite(kem, kdf, 3)
    lens = [len(p) for p in r["pt"]]
    # base mode through the single-shot device forms
    want = [s.seal(s.key_schedule(0, bytes(k["ss"][i]), r["info"][i]), 0, r["pt"][i], r["aad"][i]) for i in range(N)]
    d = dev.HpkeSuiteDevice(kem, kdf, 3)
    info, aad, pt = dev.Ragged(r["info"]), dev.Ragged(r["aad"]), dev.Ragged(r["pt"])
    enc, ct, ok = d.seal_single(0, _t(k["pkR"]), _t(k["ikmE"]), pt, aad, info)
    assert ok.cpu().numpy().all() and (enc.cpu().numpy() == k["enc"]).all()
    got = _split(ct, lens, 16)
    assert [i for i in range(N) if got[i] != want[i]] == []
    back, ok = d.open_single(0, _t(k["skR"]), enc, ct, pt, aad, info)
    assert ok.cpu().numpy().all() and _split(back, lens) == r["pt"]
    # ... and through the host forms
    h = api.HpkeSuite(kem, kdf, 3)
    enc_h, ct_h, ok = h.seal_single(0, k["pkR"], k["ikmE"], r["pt"], r["aad"], r["info"])
    assert ok.all() and (enc_h == k["enc"]).all() and ct_h == want
    back, ok = h.open_single(0, k["skR"], enc_h, ct_h, r["aad"], r["info"])
    assert ok.all() and back == r["pt"]
    # auth_psk through setup + Seal / Open on the context rows
    ks = [s.key_schedule(3, bytes(k["ass"][i]), r["info"][i], r["psk"][i], r["psk_id"][i]) for i in range(N)]
    rows = _rows([s.context_row(x) for x in ks])
    seq = [i * 3 for i in range(N)]
    enc, ctx, ok = h.setup_sender(3, k["pkR"], k["ikmE"], r["info"], r["psk"], r["psk_id"], k["skS"], k["pkS"])
    assert ok.all() and (enc == k["aenc"]).all() and (ctx == rows).all()
    ctx_r, ok = h.setup_receiver(3, k["skR"], enc, r["info"], r["psk"], r["psk_id"], k["pkS"])
    assert ok.all() and (ctx_r == rows).all()
    want = [s.seal(ks[i], seq[i], r["pt"][i], r["aad"][i]) for i in range(N)]
    assert h.seal(ctx, r["pt"], r["aad"], seq) == want
    back, ok = h.open(ctx_r, want, r["aad"], seq)
    assert ok.all() and back == r["pt"]


# ---- failures ------------------------------------------------------------------------------------------------------------------
def small_batch(kem, n):
    k = kem_reference(kem)
    return {name: k[name][:n] for name in ("pkR", "skR", "ikmE", "enc", "ss")}


def test_open_refuses_forgeries(api):
    n, bad_at = 70, (0, 63, 64, 69)
    k, h, s = small_batch(0x20, n), api.HpkeSuite(0x20, 1, 3), hc.Suite(0x20, 1, 3)
    rng = np.random.default_rng(70)
    pts = [rng.integers(0, 256, 5 + i, dtype=np.uint8).tobytes() for i in range(n)]
    aads = [rng.integers(0, 256, 1 + i % 9, dtype=np.uint8).tobytes() for i in range(n)]
    enc, ctx, ok = h.setup_sender(0, k["pkR"], k["ikmE"])
    assert ok.all()
    seq = list(range(n))
    cts = h.seal(ctx, pts, aads, seq)
    assert cts == [s.seal(s.key_schedule(0, bytes(k["ss"][i]), b""), i, pts[i], aads[i]) for i in range(n)]
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]
    for what in ("ciphertext", "tag", "aad", "seq"):
        c, a, q = list(cts), list(aads), list(seq)
        for i in bad_at:
            if what == "ciphertext":
                c[i] = flip(c[i], 0)
            elif what == "tag":
                c[i] = flip(c[i], len(c[i]) - 1)
            elif what == "aad":
                a[i] = flip(a[i], 0)
            else:
                q[i] += 1
        got, ok = h.open(ctx, c, a, q)
        assert ok.tolist() == [0 if i in bad_at else 1 for i in range(n)], what
        assert got == [bytes(len(pts[i])) if i in bad_at else pts[i] for i in range(n)], what
    # the single-shot form refuses a forged tag in the same way
    _, c, _ = h.seal_single(0, k["pkR"], k["ikmE"], pts, aads)
    for i in bad_at:
        c[i] = flip(c[i], len(c[i]) - 1)
    got, ok = h.open_single(0, k["skR"], enc, c, aads)
    assert ok.tolist() == [0 if i in bad_at else 1 for i in range(n)]
    assert got == [bytes(len(pts[i])) if i in bad_at else pts[i] for i in range(n)]


@pytest.mark.parametrize("kem", KEMS)
def test_kem_failure_propagates(api, kem):
    n, bad_at = 66, (1, 64)
    k, h = small_batch(kem, n), api.HpkeSuite(kem, 1 if kem == 0x20 else 3, 3)
    low = hp.low_order_points(kem)
    pkR = k["pkR"].copy()
    pkR[1], pkR[64] = np.frombuffer(low[1], np.uint8), np.frombuffer(low[2], np.uint8)
    pts = [bytes([i]) * (i % 40) for i in range(n)]
    enc0, ctx0, _ = h.setup_sender(0, k["pkR"], k["ikmE"])
    enc, ctx, ok = h.setup_sender(0, pkR, k["ikmE"])
    want_ok = [0 if i in bad_at else 1 for i in range(n)]
    assert ok.tolist() == want_ok
    for i in range(n):
        assert (enc[i].any(), ctx[i].any()) == (False, False) if i in bad_at else ((enc[i] == enc0[i]).all() and (ctx[i] == ctx0[i]).all()), i
    _, ct0, _ = h.seal_single(0, k["pkR"], k["ikmE"], pts)
    enc, ct, ok = h.seal_single(0, pkR, k["ikmE"], pts)
    assert ok.tolist() == want_ok and ct == [bytes(len(pts[i]) + 16) if i in bad_at else ct0[i] for i in range(n)]
    assert not enc[1].any() and not enc[64].any() and (enc[2] == enc0[2]).all()
    _, out0, _ = h.export_single(0, k["pkR"], k["ikmE"], None, 48)
    enc, out, ok = h.export_single(0, pkR, k["ikmE"], None, 48)
    assert ok.tolist() == want_ok and all((not out[i].any()) if i in bad_at else (out[i] == out0[i]).all() for i in range(n))
    # a receiver that is handed a low-order enc
    encs = enc0.copy()
    encs[1] = np.frombuffer(low[0], np.uint8)
    ctx_r, ok = h.setup_receiver(0, k["skR"], encs)
    assert ok.tolist() == [0 if i == 1 else 1 for i in range(n)] and not ctx_r[1].any() and (ctx_r[0] == ctx0[0]).all() and (ctx_r[2] == ctx0[2]).all()
    pt, ok = h.open_single(0, k["skR"], encs, ct0)
    assert ok.tolist() == [0 if i == 1 else 1 for i in range(n)] and pt == [bytes(len(p)) if i == 1 else p for i, p in enumerate(pts)]


def test_psk_rule_is_a_mask(api):
    n = 66
    k, h, s = small_batch(0x20, n), api.HpkeSuite(0x20, 1, 3), hc.Suite(0x20, 1, 3)
    psk, psk_id = [b"k" * (8 + i) for i in range(n)], [b"id%d" % i for i in range(n)]
    psk[5], psk_id[64] = b"", b""
    enc, ctx, ok = h.setup_sender(1, k["pkR"], k["ikmE"], None, psk, psk_id)
    assert ok.tolist() == [0 if i in (5, 64) else 1 for i in range(n)]
    for i in range(n):
        if i in (5, 64):
            assert not enc[i].any() and not ctx[i].any()
        else:
            assert (enc[i] == k["enc"][i]).all() and ctx[i].tobytes() == s.context_row(s.key_schedule(1, bytes(k["ss"][i]), b"", psk[i], psk_id[i])), i
    ctx_r, ok = h.setup_receiver(1, k["skR"], k["enc"], None, psk, psk_id)
    assert ok.tolist() == [0 if i in (5, 64) else 1 for i in range(n)] and (ctx_r == ctx).all()
    _, _, ok = h.setup_sender(1, k["pkR"], k["ikmE"])        # no psk at all in a psk mode: every item fails
    assert not ok.any()


def test_sequence_numbers_reach_the_high_nonce_words(api):
    k, h, s = small_batch(0x20, 4), api.HpkeSuite(0x20, 3, 3), hc.Suite(0x20, 3, 3)
    seq = [2**32, 2**64 - 1, 2**32 - 1, 2**63]
    pts, aads = [b"sequence %d" % q for q in seq], [b"a", b"", b"bc", b"def"]
    _, ctx, ok = h.setup_sender(0, k["pkR"], k["ikmE"])
    ks = [s.key_schedule(0, bytes(k["ss"][i]), b"") for i in range(4)]
    cts = h.seal(ctx, pts, aads, np.array(seq, np.uint64))
    assert ok.all() and cts == [s.seal(ks[i], seq[i], pts[i], aads[i]) for i in range(4)]
    got, ok = h.open(ctx, cts, aads, np.array(seq, np.uint64))
    assert ok.all() and got == pts


@pytest.mark.parametrize("kdf", KDFS)
def test_export_lengths_and_contexts(api, dev, kdf):
    k, h, s = small_batch(0x20, 3), api.HpkeSuite(0x20, kdf, 0xFFFF), hc.Suite(0x20, kdf, 0xFFFF)
    rng = np.random.default_rng(kdf)
    exps = [b"", b"x", rng.integers(0, 256, 150, dtype=np.uint8).tobytes()]
    _, ctx, ok = h.setup_sender(0, k["pkR"], k["ikmE"])
    ks = [s.key_schedule(0, bytes(k["ss"][i]), b"") for i in range(3)]
    assert ok.all() and [c.tobytes() for c in ctx] == [s.context_row(x) for x in ks]
    d = dev.HpkeSuiteDevice(0x20, kdf, 0xFFFF)
    for L in (1, 33, 64, 200):
        want = _rows([s.export(ks[i], exps[i], L) for i in range(3)])
        assert (h.export(ctx, exps, L) == want).all(), L
        assert (d.export(_t(ctx), dev.Ragged(exps), L).cpu().numpy() == want).all(), L
        enc, out, ok = h.export_single(0, k["pkR"], k["ikmE"], exps, L)
        assert ok.all() and (out == want).all(), L
    assert (h.export(ctx, None, 16) == _rows([s.export(x, b"", 16) for x in ks])).all()


# ---- the host pipeline's ragged outputs: chunk boundaries, shards and its three copy routes -------------------------------------
N_PIPE = 300   # two chunks of 256 + 44 items at CIRCL_HIP_HOST_CHUNK = 8; three shards of 100 on three logical devices


@pytest.fixture(scope="module")
def pipe(api):
    """keys of N_PIPE items (the first 130 from the DHKEM reference, the rest derived from random ikm) and this process's own run
    with the default settings -- one chunk, the zero-copy route -- computed once and shared"""
    import hpke_ctx_worker as hw
    k = kem_reference(0x20)
    rng = np.random.default_rng(300)
    ikmR, ikmE = (np.concatenate([k[name], rng.integers(0, 256, (N_PIPE - N, 32), dtype=np.uint8)]) for name in ("ikmR", "ikmE"))
    skR, pkR = api.hpke_dhkem_derive_keypair(0x20, ikmR)
    assert (skR[:N] == k["skR"]).all() and (pkR[:N] == k["pkR"]).all()
    keys = dict(pkR=pkR, skR=skR, ikmE=ikmE)
    return keys, hw.run(api, pkR, skR, ikmE, 0)


def _check_pipeline_run(o, keys, base):
    """what every configuration asserts about one run of hpke_ctx_worker.run"""
    import hpke_ctx_worker as hw
    pts, aads, seq = hw.inputs(N_PIPE)
    lens = [len(p) for p in pts]
    assert lens[0] == lens[255] == lens[256] == lens[296] == 0 and lens[299] == 3
    # byte for byte this process's run with the default settings
    for name in ("ct", "pt", "ct1", "pt1", "ct_noaad", "fpt", "tags", "enc", "enc1", "ctx", "ctx_r", "ok_s", "ok_r", "ok", "ok1", "ok1r", "fok"):
        assert o[name].shape == base[name].shape and (o[name] == base[name]).all(), name
    assert all(o[name].all() for name in ("ok_s", "ok_r", "ok", "ok1", "ok1r"))
    assert o["pt"].tobytes() == b"".join(pts) and o["pt1"].tobytes() == b"".join(pts)
    assert o["ct"].size == sum(lens) + 16 * N_PIPE and o["tags"].size == 16 * N_PIPE
    # the checker at both ends and on both sides of the chunk boundary
    s = hc.Suite(*hw.SUITE)
    ct, ct1, ct_noaad, tags = _split(o["ct"], lens, 16), _split(o["ct1"], lens, 16), _split(o["ct_noaad"], lens, 16), _split(o["tags"], [0] * N_PIPE, 16)
    for i in (0, 255, 256, 299):
        enc, ks = s.setup_sender(0, bytes(keys["pkR"][i]), bytes(keys["ikmE"][i]), b"")
        assert bytes(o["enc"][i]) == enc and bytes(o["ctx"][i]) == s.context_row(ks), i
        assert ct[i] == s.seal(ks, seq[i], pts[i], aads[i]) and ct_noaad[i] == s.seal(ks, seq[i], pts[i], b""), i
        assert ct1[i] == s.seal(ks, 0, pts[i], aads[i]) and tags[i] == s.seal(ks, seq[i], b"", aads[i]), i
    # forged tags: ok = 0 and zeros of the right length there, every other item intact
    assert o["fok"].tolist() == [0 if i in hw.FORGED else 1 for i in range(N_PIPE)]
    assert _split(o["fpt"], lens) == [bytes(lens[i]) if i in hw.FORGED else pts[i] for i in range(N_PIPE)]
    # nothing was written before or behind an output blob
    assert o["guards"].all() and o["guarded_same"].all()
    # an Open over rows of tags, Export, and the pass in mode 3: byte for byte the default run's, and the checker at both ends and on both
    # sides of the shard boundaries and of the chunk boundary
    more = ("tok", "exp", "enc_x", "exp1", "exp1r", "ok_x", "ok_xr", "skS", "pkS", "enc3", "ctx3", "ctx3_r", "ok3_s", "ok3_r", "enc3_1", "ct3_1", "pt3_1",
            "ok3_1", "ok3_1r", "enc3_x", "exp3", "exp3_r", "ok3_x", "ok3_xr")
    for name in more:
        assert o[name].shape == base[name].shape and (o[name] == base[name]).all(), name
    assert all(o[name].all() for name in more if name.startswith("ok"))
    assert o["tok"].tolist() == [0 if i == hw.FORGED_TAG else 1 for i in range(N_PIPE)]
    assert (o["exp1r"] == o["exp1"]).all() and (o["enc_x"] == o["enc"]).all() and o["exp"].shape == (N_PIPE, hw.EXPORT_L)
    assert (o["ctx3_r"] == o["ctx3"]).all() and (o["exp3_r"] == o["exp3"]).all() and o["pt3_1"].tobytes() == b"".join(pts)
    assert (o["enc3_1"] == o["enc3"]).all() and (o["enc3_x"] == o["enc3"]).all()
    exps, (_, infos, psks, ids), ct3 = hw.exporter_contexts(N_PIPE), hw.auth_psk_inputs(N_PIPE), _split(o["ct3_1"], lens, 16)
    for i in (0, 99, 100, 199, 200, 255, 256, 299):
        _, ks = s.setup_sender(0, bytes(keys["pkR"][i]), bytes(keys["ikmE"][i]), b"")
        assert bytes(o["exp"][i]) == bytes(o["exp1"][i]) == s.export(ks, exps[i], hw.EXPORT_L), i
        enc, ks = s.setup_sender(3, bytes(keys["pkR"][i]), bytes(keys["ikmE"][i]), infos[i], psks[i], ids[i], skS=bytes(o["skS"][i]))
        assert bytes(o["enc3"][i]) == enc and bytes(o["ctx3"][i]) == s.context_row(ks), i
        assert ct3[i] == s.seal(ks, 0, pts[i], aads[i]) and bytes(o["exp3"][i]) == s.export(ks, exps[i], hw.EXPORT_L), i


def test_pipeline_default_run_takes_the_checks(pipe):
    keys, base = pipe
    _check_pipeline_run(base, keys, base)


@pytest.mark.parametrize("env,device", [({"CIRCL_HIP_HOST_CHUNK": "8"}, 0), ({"CIRCL_HIP_HOST_CHUNK": "8", "CIRCL_HIP_LOGICAL_DEVICES": "3"}, -1),
                                        ({"CIRCL_HIP_ZEROCOPY_KB": "0"}, 0)], ids=["chunks", "chunks-in-shards", "merged-copy"])
def test_pipeline_routes_agree(pipe, tmp_path, env, device):
    import os
    import subprocess
    import sys
    keys, base = pipe
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **keys)
    e = {k: v for k, v in os.environ.items() if k not in ("CIRCL_HIP_HOST_CHUNK", "CIRCL_HIP_ZEROCOPY_KB", "CIRCL_HIP_LOGICAL_DEVICES")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hpke_ctx_worker.py"), str(device), src, dst], check=True, env=e,
                   timeout=300)
    _check_pipeline_run(np.load(dst), keys, base)


def test_seal_into_page_locked_blobs(api):
    """caller blobs from circl_hip_alloc_host are not staged: the pipeline copies straight from / to their ragged addresses"""
    import ctypes as C
    import hpke_ctx_worker as hw
    n = 70
    k, h = small_batch(0x20, n), api.HpkeSuite(*hw.SUITE)
    pts, aads, seq = (x[:n] for x in hw.inputs(n))
    _, ctx, ok = h.setup_sender(0, k["pkR"], k["ikmE"])
    want = b"".join(h.seal(ctx, pts, aads, seq))
    (pb, off), (ab, ao), sq = api._blob(pts), api._blob(aads), np.array(seq, np.uint64)
    P, G = int(off[n]), hw.GUARD
    L = h.L
    mem_pt, mem_ct = L.circl_hip_alloc_host(P + 16), L.circl_hip_alloc_host(P + 16 * n + 2 * G)
    assert mem_pt and mem_ct
    try:
        C.memmove(mem_pt, pb.ctypes.data, P)
        C.memset(mem_ct, hw.FILL, P + 16 * n + 2 * G)
        rc = L.circl_hip_hpke_seal(3, api._p(ctx), h.CS, api._p(sq), mem_pt, api._p(off), api._p(ab), api._p(ao), mem_ct + G, n, 0)
        got = C.string_at(mem_ct, P + 16 * n + 2 * G)
    finally:
        L.circl_hip_free_host(mem_pt)
        L.circl_hip_free_host(mem_ct)
    assert rc == 0 and ok.all()
    assert got[G:-G] == want and got[:G] == bytes([hw.FILL]) * G and got[-G:] == bytes([hw.FILL]) * G
