"""The transcript's kernels on the GPU (include/pbf.h "Fiat-Shamir"; csrc/transcript.hip:
k_keccak_batch, k_keccak_tree_level, k_plonk_chain, k_plonk_rho) against the pure-Python model
tests/transcript_expect.py, through pbf_keccak256_batch and pbf_plonk_challenges_bn254.

The transcript hashes whatever bytes it is given, so the "proofs" here are seeded random values: no
circuit, no prover. Model values are computed once per module and shared."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transcript_expect as T  # noqa: E402

pytestmark = pytest.mark.gpu
R = T.R
# 135: both padding bits in one byte; 136: a block of padding only; 137 / 271..273: the second and third block
LENGTHS = [0, 1, 135, 136, 137, 271, 272, 273]
COUNTS = [1, 63, 64, 65]  # across a wave boundary


def _msgs(n, count):
    rng = random.Random(1000 * n + count)
    return [bytes(rng.randrange(256) for _ in range(n)) for _ in range(count)]


@pytest.mark.parametrize("n", LENGTHS)
def test_keccak256_batch_against_the_model(ctx, n):
    msgs = _msgs(n, max(COUNTS))
    want = [T.H(m) for m in msgs]
    for count in COUNTS:
        for pitch in (n + 16 - n % 8, n + 3):  # lanes read whole, and byte by byte: both above len
            assert ctx.keccak256_batch(msgs[:count], pitch=pitch) == want[:count], (count, pitch)


def test_keccak256_batch_dev_form_and_errors(ctx):
    import torch

    import pbf

    msgs = _msgs(137, 65)
    pitch = 144
    buf = np.zeros(65 * pitch, dtype=np.uint8)
    for i, m in enumerate(msgs):
        buf[i * pitch:i * pitch + 137] = np.frombuffer(m, dtype=np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.zeros(65 * 32, dtype=torch.uint8, device="cuda")
    ctx.keccak256_batch_dev(d_in.data_ptr(), 65, 137, pitch, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().tobytes()
    assert [out[32 * i:32 * i + 32] for i in range(65)] == [T.H(m) for m in msgs]
    for call in (lambda: ctx.keccak256_batch([]), lambda: ctx.keccak256_batch(msgs[:2], pitch=136),
                 lambda: ctx.keccak256_batch_dev(0, 1, 8, 8, d_out.data_ptr()),
                 lambda: ctx.keccak256_batch_dev(d_in.data_ptr(), 1, 8, 8, 0)):
        with pytest.raises(pbf.PbfError) as ei:
            call()
        assert ei.value.code == pbf.PBF_EINVAL
    assert ctx.keccak256_batch([b"abc"])[0].hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


# ---------------------------------------------------------------- the PLONK transcript
H0 = T.H(b"a circuit digest for the transcript kernels")


def _proof(rng):
    """9 pairs of coordinates below 2^254 and 7 fields below r: bytes to hash, not a proof."""
    return [(rng.randrange(1 << 254), rng.randrange(1 << 254)) for _ in range(9)], [rng.randrange(R) for _ in range(7)]


@pytest.fixture(scope="module")
def world():
    """21 proofs, two of them special, their public inputs for every npub, and the model's values."""
    rng = random.Random(0xF5)
    proofs = [_proof(rng) for _ in range(21)]
    proofs[3][0][4] = None  # the identity as t_lo: 64 zero bytes
    proofs[4][1][5] = (1 << 256) - 1 - rng.randrange(1 << 64)  # a field >= r: hashed as given
    pubs = {npub: [[rng.randrange(R) for _ in range(npub)] for _ in range(21)] for npub in (0, 1, 4, 5, 17)}
    pubs[5][0][4] = R - 1
    chains = {npub: [T.proof_chain(H0, pub, pts, fs) for pub, (pts, fs) in zip(pubs[npub], proofs)] for npub in pubs}
    return proofs, pubs, chains


# count: single, full and ragged groups of 4 on one and two levels of the tree over the t6
@pytest.mark.parametrize("count", [1, 2, 4, 5, 16, 17, 21])
@pytest.mark.parametrize("npub", [0, 1, 4, 5, 17])
def test_challenges_against_the_model(ctx, world, count, npub):
    proofs, pubs, chains = world
    chal, u, rho = ctx.plonk_challenges_bn254(H0, proofs[:count], pubs[npub][:count])
    want = chains[npub][:count]
    assert chal == [T.chal5(c) for c, _ in want]
    assert u == [c["u"] for c, _ in want]
    assert rho == T.batch_rhos([t for _, t in want])
    assert all(0 < x < R for x in rho)


def test_challenges_without_rho_and_their_errors(ctx, world):
    import pbf

    proofs, pubs, chains = world
    chal, u, rho = ctx.plonk_challenges_bn254(H0, proofs[:5], pubs[4][:5], rho=False)
    assert rho is None and chal == [T.chal5(c) for c, _ in chains[4][:5]] and u == [c["u"] for c, _ in chains[4][:5]]
    other = ctx.plonk_challenges_bn254(T.H(b"another digest"), proofs[:5], pubs[4][:5])
    assert all(a != b for a, b in zip(other[0], chal))
    bad = [list(p) for p in pubs[4][:5]]
    bad[2][3] = R
    for call in (lambda: ctx.plonk_challenges_bn254(H0, [], []), lambda: ctx.plonk_challenges_bn254(H0, proofs[:5], bad)):
        with pytest.raises(pbf.PbfError) as ei:
            call()
        assert ei.value.code == pbf.PBF_EINVAL
    lib, z = ctx.lib, np.zeros(72, dtype=np.uint64)
    d = np.frombuffer(H0, dtype=np.uint8).copy()
    p8 = d.ctypes.data_as(pbf._p8)
    for args in ((None, 1, pbf._ptr(z), pbf._ptr(z), None, 0, pbf._ptr(z), pbf._ptr(z), None),
                 (p8, 1, None, pbf._ptr(z), None, 0, pbf._ptr(z), pbf._ptr(z), None),
                 (p8, 1, pbf._ptr(z), pbf._ptr(z), None, 1, pbf._ptr(z), pbf._ptr(z), None),
                 (p8, (1 << 20) + 1, pbf._ptr(z), pbf._ptr(z), None, 0, pbf._ptr(z), pbf._ptr(z), None)):
        assert lib.pbf_plonk_challenges_bn254(ctx.h, *args) == pbf.PBF_EINVAL
    assert ctx.plonk_challenges_bn254(H0, proofs[:5], pubs[4][:5], rho=False)[0] == chal
