"""The matrix sampler's FIFO flush schedule (parse_shake128_block_fifo, mlkem_kernels.h: 32 entries = 64 bytes at a time, checks after
candidates 32, 64, 96 and 112 of a block; stragglers of a fourth block parked with up to 31 pending entries and adopted by the PRF pass)
on inputs that sit on its edges, byte for byte against the oracle and, row by row, against the oracle's sampler through
circl_hip_kyber_sample_uniform.  The inputs are found on the CPU when the module's fixture runs (tests/kem_flush_inputs.py, proven by
tests/test_kem_flush_inputs.py): for K = 2, 3, 4 a stream whose 256th accept falls on candidate 64, 96, 112 of block 3 and one after each
(112 = the last candidate of block 3, 113 = the first of block 4), streams with exactly 32 entries pending at the check after candidate 32
of block 3 and one candidate later (the 256th accept itself cannot fall there: probability 9e-24), stragglers short by 1 and by 9 or
more, two in one key, one on lane 0 and one on the last active lane of one group.  ML-KEM-512 (eta1 = 3) takes the plain fourth-block
loop with the same inputs.  Batches of 1, G - 1, G, G + 1, 2 G + 3 items with the inputs in the first, the last and the group-boundary
items; per-item keys, one key, a key table; every batch route the environment can force (tests/test_gpu_round3.py, test_gpu_round4.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kem_flush_inputs as fi
import kem_flush_worker as worker
from circl_amd import hostapi
from oracle import orc
from test_gpu_round3 import KEM_ROUTE_IDS, KEM_ROUTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the routes of test_gpu_round3.py::test_kem_batch_routes, and the one-launch chain kernels off / widened (test_gpu_round4.py)
ROUTES = KEM_ROUTES[1:] + [{"CIRCL_HIP_KEM_CHAIN": "0", "CIRCL_HIP_KEM_CHAIN_ENCAPS": "0"}, {"CIRCL_HIP_KEM_CHAIN": "12", "CIRCL_HIP_KEM_CHAIN_ENCAPS": "12"}]
ROUTE_IDS = KEM_ROUTE_IDS[1:] + ["resident-chain-off", "resident-chain-wide"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    found = worker.find_inputs()                       # fails if a shape is not found within 2^22 tries
    path = str(tmp_path_factory.mktemp("kem_flush") / "inputs.json")
    with open(path, "w") as f:
        json.dump(found, f)
    return found, path


@pytest.mark.parametrize("param", [512, 768, 1024])
def test_flush_edges_default_routes(param, inputs):
    K = fi.PARAM_K[param]
    assert worker.run(param, inputs[0]) == len(fi.placements(K, len(fi.SHAPES)))


@pytest.mark.parametrize("env_extra", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("param", [512, 768, 1024])
def test_flush_edges_on_every_route(env_extra, param, inputs):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kem_flush_worker.py"), inputs[1], str(param)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    want = "kem flush ok %d %d" % (param, len(fi.placements(fi.PARAM_K[param], len(fi.SHAPES))))
    assert r.returncode == 0 and want in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]


@pytest.mark.parametrize("K", [2, 3, 4])
def test_sample_rows_on_the_flush_edges(K, inputs):
    """every stream of every found rho through the unit-level sampler (lane = stream, the XY_ARG form of sample_matrix_scratch): the streams
    that carry a shape in the first and the last lane of launches of 1, 63, 64, 65 and 131 streams, every row against the oracle's"""
    found = inputs[0][str(K)]
    rhos = [bytes.fromhex(h) for h in found["rho"].values()] + [fi.mlkem_rho(K, bytes.fromhex(h)) for h in found["d"].values()]
    rhos += [fi.mlkem_rho(K, d) for d in fi.ordinary(K, 40, 99)]   # (enough ordinary streams to fill the longest launch)
    special, plain = [], []
    for rho in dict.fromkeys(rhos):
        for (x, y), (end, a256, a257, a336) in fi.profile(rho, K).items():
            edge = end in (288, 289, 320, 321, 336, 337) or a336 < 256 or a256 == 224 or (a256 == 223 and a257 == 224)
            (special if edge else plain).append((rho, x, y))
    assert len(special) >= len(fi.SHAPES) and len(plain) >= 129
    want = {}

    def check(batch):
        seeds = np.frombuffer(b"".join(s[0] for s in batch), np.uint8).reshape(len(batch), 32)
        xy = np.array([[s[1], s[2]] for s in batch], np.uint8)
        got = hostapi.kyber_sample_uniform(seeds, xy)
        for i, s in enumerate(batch):
            if s not in want:
                want[s] = np.asarray(orc.kyber_uniform(s[0], s[1], s[2]), np.int16)
                assert (want[s] == fi.sample(*s)).all()
            assert (got[i] == want[s]).all(), (K, len(batch), i, s[0].hex(), s[1], s[2])

    for n in (1, 63, 64, 65, 131):
        for i in range(0, len(special), 2):
            a, b = special[i], special[(i + 1) % len(special)]
            check([a] if n == 1 else [a] + plain[:n - 2] + [b])
        if n == 1:
            for s in special[1::2]:
                check([s])
    check(special + plain)                              # all of them in one launch
