"""CPU tier: the inputs tests/test_gpu_kem_flush.py runs the kernels on exist and are what they claim (tests/kem_flush_inputs.py): the model of
the rejection sampler is the oracle's sampler, the search finds every shape for every parameter set well inside its 2^22 tries, and a found
rho / seed has its shape when the candidates are counted again here, byte by byte."""
import hashlib

import numpy as np
import pytest

import kem_flush_inputs as fi
from oracle import orc


def _candidates(rho, x, y, n):
    """the first n 12-bit candidates of XOF(rho || x || y), one at a time"""
    buf = hashlib.shake_128(rho + bytes([x, y])).digest(3 * ((n + 1) // 2))
    out = []
    for i in range(0, len(buf), 3):
        out.append(buf[i] | ((buf[i + 1] & 15) << 8))
        out.append((buf[i + 1] >> 4) | (buf[i + 2] << 4))
    return out[:n]


@pytest.fixture(scope="module", params=[2, 3, 4])
def found(request):
    K = request.param
    return K, fi.search(K, False), fi.search(K, True)


def test_model_is_the_oracle_sampler():
    for k in range(6):
        rho = hashlib.sha3_256(b"model %d" % k).digest()
        for x, y in ((0, 0), (1, 2), (3, 3)):
            assert fi.sample(rho, x, y).tolist() == list(orc.kyber_uniform(rho, x, y))


def test_every_shape_is_found_and_holds(found):
    K, rhos, ds = found
    assert set(rhos) == set(ds) == set(fi.SHAPES)
    for name in fi.SHAPES:
        for rho in (rhos[name], fi.mlkem_rho(K, ds[name])):
            assert fi.SHAPES[name](fi.profile(rho, K), K), (K, name)


def test_shapes_counted_candidate_by_candidate(found):
    K, rhos, _ = found
    ends = {"finish_288": 288, "finish_289": 289, "finish_320": 320, "finish_321": 321, "finish_336": 336, "finish_337": 337}
    for name, c in ends.items():
        hits = 0
        for x in range(K):
            for y in range(K):
                acc = [v < fi.KQ for v in _candidates(rhos[name], x, y, c)]
                hits += sum(acc) == 256 and acc[-1]          # the 256th coefficient is accepted exactly on candidate c
        assert hits >= 1, (K, name)
    short = [sum(v < fi.KQ for v in _candidates(rhos["short_by_1"], x, y, 336)) for x in range(K) for y in range(K)]
    assert 255 in short
    short = [sum(v < fi.KQ for v in _candidates(rhos["short_by_9_or_more"], x, y, 336)) for x in range(K) for y in range(K)]
    assert min(short) <= 247
    at256 = [sum(v < fi.KQ for v in _candidates(rhos["pending_32_at_256"], x, y, 256)) for x in range(K) for y in range(K)]
    assert 224 in at256                                       # 192 flushed at the check after candidate 224, 32 pending at candidate 256


def test_candidate_256_is_out_of_reach():
    # the 256th accept on candidate 32 of block 3 needs all of the first 256 candidates accepted (module docstring of kem_flush_inputs)
    assert (fi.KQ / 4096) ** 256 * 16 * fi.MAX_TRIES < 1e-15


def test_placements_cover_every_shape_at_every_size():
    for K in (2, 3, 4):
        G, sizes = fi.batch_sizes(K)
        assert G == 64 // (K * K) and sizes == (1, G - 1, G, G + 1, 2 * G + 3)
        n_shapes = len(fi.SHAPES)
        for n in sizes:
            placed = [s for m, places in fi.placements(K, n_shapes)[:-1] if m == n for s in places.values()]
            assert sorted(placed) == list(range(n_shapes)), (K, n)
            firsts = [min(places) for m, places in fi.placements(K, n_shapes) if m == n]
            lasts = [max(places) for m, places in fi.placements(K, n_shapes) if m == n]
            assert set(firsts) == {0} and n - 1 in lasts
