"""The 2^20 default plan "10,10" with its intermediate tile-major (ntt_gl.hpp SP 2, selected by
ntt_launch.hip gl_blocked): the first pass stores y(j, k) at Yb[k >> 3][j][k & 7] with its
post-twiddle table in the same order, the second pass reads each tile as one contiguous block.
2^20 is the smallest size at which "10,10" exists. Only plain forward transforms take the
layout: the inverse and the round trip run the natural-order kernels and must agree with it.

Inputs: random, the carry / borrow edge values of test_ntt_gl_valu_gpu.py, all p-1, and unit
impulses at 0, 7, 8, 1023, 1024, 8191, 8192 and n-1 (input x[j + 1024 r]: the positions
straddle the k & 7, block and column boundaries of the layout; every output of an impulse is
one twiddle power, so a misplaced block or table entry shows).

Batches 1, 4, 8, 9 and 13 (one group; two streams; a ragged last group; a scratch slot reused
by a third and fourth group), two calls back to back, against the same polynomials transformed
singly. The scratch slots are gl_scratch_pitch = 128 block pitches apart per polynomial; the
block pitch kept is the dense 8192 (a padded pitch measured no faster),
so pitch and tile size coincide and there is no pad for batch 9 to make visible."""
import numpy as np
import pytest

import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
LOGN = 20
N = 1 << LOGN
W = pow(7, (GOLD - 1) // N, GOLD)
EDGE_GL = [0, 1, 2, GOLD - 1, GOLD - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) - 1,
           GOLD - (1 << 32), GOLD - (1 << 32) + 1, (1 << 64) - (1 << 33), 0xFFFFFFFE00000001, 0x00000000FFFFFFFF,
           0x7FFFFFFF80000000]  # the values of tests/test_ntt_gl_valu_gpu.py
IMPULSES = (0, 7, 8, 1023, 1024, 8191, 8192, N - 1)


def poly(seed):
    return np.random.default_rng(seed).integers(0, GOLD, N, dtype=np.uint64)


def inputs():
    rng = np.random.default_rng(2900)
    ins = {"random": poly(2901),
           "edge": np.array(EDGE_GL, dtype=np.uint64)[rng.integers(0, len(EDGE_GL), N)],
           "all_p_minus_1": np.full(N, GOLD - 1, dtype=np.uint64)}
    for pos in IMPULSES:
        a = np.zeros(N, dtype=np.uint64)
        a[pos] = 1
        ins[f"impulse_{pos}"] = a
    return ins


_REFS = {}


def refs():
    """name -> (input, forward) by oracle.ntt_iter, computed once"""
    if not _REFS:
        for k, a in inputs().items():
            _REFS[k] = (a, oracle.ntt_iter(GOLD, W, a))
            for x in _REFS[k]:
                x.setflags(write=False)
    return _REFS


_SINGLE = {}


def single(c, seed):
    """(polynomial of that seed, its forward transform as a batch of one), computed once"""
    if seed not in _SINGLE:
        a = poly(seed)
        _SINGLE[seed] = (a, c.ntt(GOLD, W, a))
        for x in _SINGLE[seed]:
            x.setflags(write=False)
    return _SINGLE[seed]


def test_default_plan_vs_oracle(ctx):
    for name, (a, fwd) in refs().items():
        got = ctx.ntt(GOLD, W, a)
        assert np.array_equal(got, fwd), (name, "forward")
        assert np.array_equal(ctx.ntt(GOLD, W, got, inverse=True), a), (name, "round trip")
    for name in ("random", "edge"):
        a = refs()[name][0]
        assert np.array_equal(ctx.ntt(GOLD, W, a, inverse=True), oracle.ntt_iter(GOLD, W, a, inverse=True)), (name, "inverse")


def batched_twice(c, batch):
    """Two batched forward calls back to back on one stream, no synchronisation between them
    (a scratch slot reused before its reader has finished shows), against the single transforms"""
    import torch

    seeds = [[3000 + 16 * s + i for i in range(batch)] for s in range(2)]
    host = [np.stack([single(c, sd)[0] for sd in ss]) for ss in seeds]
    d_in = [torch.from_numpy(h.view(np.int64)).cuda() for h in host]
    d_out = [torch.empty_like(d) for d in d_in]
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for s in range(2):
        c.ntt_batch_dev(GOLD, W, d_in[s].data_ptr(), d_out[s].data_ptr(), N, batch, stream=stream)
    torch.cuda.synchronize()
    for s in range(2):
        got = d_out[s].cpu().numpy().view(np.uint64)
        for i, sd in enumerate(seeds[s]):
            assert np.array_equal(got[i], single(c, sd)[1]), (batch, s, i)


@pytest.mark.parametrize("batch", [1, 4, 8, 9, 13])
def test_batches_match_single(ctx, batch):
    batched_twice(ctx, batch)


@pytest.mark.parametrize("streams", [1, 3])
def test_batch9_groups_of_two(streams):
    """Groups of 2 over 1 and 3 streams: five groups, the last ragged, every slot reused"""
    c = pbf.Context(0, options={"ntt.group": "2", "ntt.streams": str(streams)})
    try:
        batched_twice(c, 9)
    finally:
        c.close()
