"""CPU test of the transcript model itself (tests/transcript_expect.py): its sponge against
hashlib.sha3_256 -- the same rate-136 sponge over the same permutation, with first padding byte 0x06
-- at the lengths around the block edges, Ethereum's two known Keccak-256 answers with padding byte
0x01, and the challenges it derives for the committed golden proofs of
tests/golden/plonk_pi_bn254.json against their record in tests/golden/plonk_fs_bn254.json
(tests/golden/gen_plonk_fs_golden.py)."""
import hashlib
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import transcript_expect as T  # noqa: E402

LENGTHS = [0, 1, 135, 136, 137, 271, 272, 273]


@pytest.mark.parametrize("n", LENGTHS)
def test_sponge_with_sha3_padding_is_hashlib_sha3_256(n):
    msg = bytes(random.Random(n).randrange(256) for _ in range(n))
    assert T.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest()


def test_keccak256_known_answers():
    assert T.H(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert T.H(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_permutation_tables_are_the_specifications():
    assert T.RC[0] == 1 and T.RC[1] == 0x8082 and T.RC[23] == 0x8000000080008008
    assert [T.ROT[x][0] for x in range(5)] == [0, 1, 62, 28, 27]


def test_tree_digest_shape_is_fixed_by_the_length():
    a, b = T.be32(1), T.be32(2)
    assert T.tree_digest(7, []) == T.H(T.u64(7) + T.u64(0) + bytes(32))
    assert T.tree_digest(7, [a]) == T.H(T.u64(7) + T.u64(1) + T.H(a))  # one item is still hashed once
    five = [a, b, a, b, a]
    assert T.tree_digest(8, five) == T.H(T.u64(8) + T.u64(5) + T.H(T.H(a + b + a + b) + T.H(a)))
    assert T.tree_digest(8, five) != T.tree_digest(7, five)


def test_challenge_reduces_mod_r_and_rho_is_never_zero():
    assert T.challenge(T.be32(T.R)) == 0 and T.challenge(T.be32(T.R + 5)) == 5
    assert T.challenge(bytes([0xFF] * 32)) == ((1 << 256) - 1) % T.R
    assert all(0 < r < T.R for r in T.batch_rhos([T.H(bytes([i])) for i in range(5)]))


GOLD_PI = os.path.join(HERE, "golden", "plonk_pi_bn254.json")
GOLD_FS = os.path.join(HERE, "golden", "plonk_fs_bn254.json")


def test_challenges_of_the_golden_proofs_are_the_recorded_ones():
    import plonk_pi_expect as E

    pi = json.load(open(GOLD_PI))["cases"]
    fs = json.load(open(GOLD_FS))["cases"]
    assert [(c["n"], c["npub"], c["mode"]) for c in fs] == [(c["n"], c["npub"], c["mode"]) for c in pi]
    t6s = []
    for c, want in zip(pi, fs):
        pub = E.case_inputs(c["n"], c["npub"], c["mode"])["pub"]
        pre = [None if p is None else tuple(p) for p in want["vk"]]
        h0 = T.circuit_digest({"reference": 0, "paper": 1}[c["mode"]], c["n"], c["npub"], 2, 3, pre, want["g2s"])
        assert h0.hex() == want["digest"]
        pts = [None if p is None or tuple(p) == (0, 0) else tuple(p) for p in c["pts"]]
        ch, t6 = T.proof_chain(h0, pub, pts, c["fields"])
        assert ch == want["challenges"]
        assert t6.hex() == want["t6"]
        t6s.append(t6)
    assert T.batch_rhos(t6s) == json.load(open(GOLD_FS))["rhos_of_all_cases_as_one_batch"]
