"""The FrodoKEM-640-SHAKE checker of tests/frodo.py against the reference's pin: the SHA-256 of the NIST KAT transcript of 100
keygen / encaps / decaps triples (kem/frodo/kat_test.go), recorded in tests/golden/frodo640shake.json.  CPU only."""
import numpy as np
import pytest

import frodo as ref

from frodo import golden, kat_seeds, kat_transcript


def test_golden_sizes_match_the_checker():
    g = golden()
    assert g["name"] == ref.NAME
    assert (g["public_key_size"], g["private_key_size"], g["ciphertext_size"], g["shared_key_size"], g["seed_size"],
            g["encapsulation_seed_size"]) == (ref.PK_BYTES, ref.SK_BYTES, ref.CT_BYTES, ref.SS_BYTES, ref.KEYSEED_BYTES, ref.ENCSEED_BYTES)


def test_checker_replays_the_kat_transcript():
    g = golden()
    entries = []
    for seed, kseed, eseed in kat_seeds(g["kat_count"]):
        pk, sk = ref.keygen(kseed)
        ct, ss = ref.encaps(pk, eseed)
        assert ref.decaps(sk, ct) == ss
        entries.append((seed, pk, sk, ct, ss))
    assert kat_transcript(g["name"], entries) == g["kat_sha256"]


@pytest.fixture(scope="module")
def pair():
    pk, sk = ref.keygen(bytes(range(48)))
    ct, ss = ref.encaps(pk, bytes(range(16)))
    return pk, sk, ct, ss


def test_round_trip_and_sizes(pair):
    pk, sk, ct, ss = pair
    assert (len(pk), len(sk), len(ct), len(ss)) == (ref.PK_BYTES, ref.SK_BYTES, ref.CT_BYTES, ref.SS_BYTES)
    assert sk[:16] == bytes(range(16)) and sk[16:16 + ref.PK_BYTES] == pk and sk[-16:] == ref.shake128(pk, 16)
    assert ref.decaps(sk, ct) == ss


@pytest.mark.parametrize("byte", [0, 9599, 9600, 9719])
def test_flipped_bit_gives_the_rejection_key(pair, byte):
    pk, sk, ct, ss = pair
    bad = bytearray(ct)
    bad[byte] ^= 1
    got = ref.decaps(sk, bytes(bad))
    assert got == ref.shake128(bytes(bad) + sk[:16], 16) and got != ss


def test_pack_and_sampler_edges():
    v = np.array([0, 1, 0x7fff, 0x8000, 0xffff, 0x4000, 0x2aaa, 0x5555], np.uint16)
    assert (ref.unpack(ref.pack(v), 8) == (v & ref.QMASK)).all()
    assert ref.pack(np.full(8, 0xffff, np.uint16)) == b"\xff" * 15
    s = ref.sample(np.arange(65536, dtype=np.uint32).astype(np.uint16)).astype(np.int16)
    assert s.min() == -12 and s.max() == 12 and s[0] == 0 and s[1] == 0
    assert s[2 * 4643] == 0 and s[2 * 4644] == 1 and s[2 * 4644 + 1] == -1
