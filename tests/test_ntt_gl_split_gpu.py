"""The two "10,10" pass kernels of the 2^20 default plan with their LDS exchanges split into
32-bit halves (ntt_gl.hpp SP 2: low words through LDS first, high words second, 33,280 B per
workgroup, three workgroups per CU). 2^20 is the only size that runs these kernels.

What the split can get wrong and the inputs that show it:
  - a half taken from the wrong round, or low and high words swapped: every low word 0 with
    random high words, every high word 0 with random low words, and low word 0xFFFFFFFF with
    high word 0 (all of them canonical: the largest is 0xFFFFFFFF00000000 = p - 1);
  - a misplaced element: unit impulses at rows 0, 1, 127, 128, 1023 of the first pass's tile
    (input x[j + 1024 r]) and at columns 7, 8 on the two sides of an 8-column tile boundary;
    every output of an impulse is one twiddle power;
  - a missing barrier between two rounds of one exchange: batch 32 called 8 times back to back,
    when every CU holds three workgroups of the two concurrent kernels, every output compared.
The default schedule of this plan is groups of 8 polynomials from batch 16 on (groups of 4 from 8
to 15): batch 9 is 4 + 4 + 1, batch 17 is 8 + 8 + 1, batch 32 four groups on two streams.

All references are oracle.ntt_iter (one polynomial) or oracle.ntt_gl_par (batches), computed
once. The round trip goes through the natural-order inverse, which this layout does not touch."""
import numpy as np
import pytest

import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
LOGN = 20
N = 1 << LOGN
W = pow(7, (GOLD - 1) // N, GOLD)
IMPULSE_ROWS = (0, 1, 127, 128, 1023)
IMPULSE_COLS = (0, 7, 8)  # 7 | 8: the boundary between the first two 8-column tiles
BIG, CALLS = 32, 8


def value_sets(batch, seed):
    """name -> [batch][N] canonical inputs"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 1 << 32, (batch, N), dtype=np.uint64)
    hi = rng.integers(0, (1 << 32) - 1, (batch, N), dtype=np.uint64)  # hi <= 2^32 - 2: canonical with any low word
    return {"random": rng.integers(0, GOLD, (batch, N), dtype=np.uint64),
            "all_p_minus_1": np.full((batch, N), GOLD - 1, dtype=np.uint64),
            "low_zero": hi << np.uint64(32),
            "high_zero": lo,
            "low_ones_high_zero": np.full((batch, N), 0xFFFFFFFF, dtype=np.uint64)}


_REFS = {}


def refs(batch):
    """name -> (input [batch][N], forward [batch][N]) by the oracle, computed once"""
    if batch not in _REFS:
        out = {}
        for name, a in value_sets(batch, 4100 + batch).items():
            fwd = oracle.ntt_gl_par(W, a.reshape(-1), batch=batch).reshape(batch, N)
            if name == "random":  # the two oracles against each other, once per batch
                assert np.array_equal(fwd[0], oracle.ntt_iter(GOLD, W, a[0]))
            out[name] = (a, fwd)
            for x in out[name]:
                x.setflags(write=False)
        _REFS[batch] = out
    return _REFS[batch]


def forward_dev(c, host, calls=1):
    """`calls` batched forward transforms of host [batch][N] back to back on one stream, each
    into its own output; returns the outputs"""
    import torch

    batch = host.shape[0]
    d_in = torch.from_numpy(np.array(host).view(np.int64)).cuda()
    d_out = [torch.empty_like(d_in) for _ in range(calls)]
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for o in d_out:
        c.ntt_batch_dev(GOLD, W, d_in.data_ptr(), o.data_ptr(), N, batch, stream=stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint64) for o in d_out]


@pytest.mark.parametrize("batch", [1, 4, 9])
def test_value_sets_vs_oracle(ctx, batch):
    for name, (a, fwd) in refs(batch).items():
        got = forward_dev(ctx, a)[0]
        assert np.array_equal(got, fwd), (batch, name)


def test_impulses(ctx):
    """x[j + 1024 r] = 1: row r of the first pass's tile, column j"""
    for r in IMPULSE_ROWS:
        for j in IMPULSE_COLS:
            a = np.zeros(N, dtype=np.uint64)
            a[j + 1024 * r] = 1
            assert np.array_equal(ctx.ntt(GOLD, W, a), oracle.ntt_iter(GOLD, W, a)), (r, j)


def test_batch32_eight_calls(ctx):
    rng = np.random.default_rng(4200)
    a = rng.integers(0, GOLD, (BIG, N), dtype=np.uint64)
    fwd = oracle.ntt_gl_par(W, a.reshape(-1), batch=BIG).reshape(BIG, N)
    for call, got in enumerate(forward_dev(ctx, a, calls=CALLS)):
        bad = np.flatnonzero((got != fwd).any(axis=1))
        assert bad.size == 0, (call, bad.tolist())


def test_batch17_ragged_third_group(ctx):
    """Default schedule at batch 17: groups of 8, 8 and 1 on two streams, the third group in the
    first group's scratch slot; two calls back to back"""
    rng = np.random.default_rng(4300)
    a = rng.integers(0, GOLD, (17, N), dtype=np.uint64)
    fwd = oracle.ntt_gl_par(W, a.reshape(-1), batch=17).reshape(17, N)
    for call, got in enumerate(forward_dev(ctx, a, calls=2)):
        bad = np.flatnonzero((got != fwd).any(axis=1))
        assert bad.size == 0, (call, bad.tolist())


@pytest.mark.parametrize("streams", [1, 3])
def test_groups_of_two(streams):
    """ntt.group 2 on 1 and 3 streams (batch 9: five groups, the last ragged), to the batch-1
    results of the default context's reference"""
    a, fwd = refs(9)["random"]
    c = pbf.Context(0, options={"ntt.group": "2", "ntt.streams": str(streams)})
    try:
        for call, got in enumerate(forward_dev(c, a, calls=2)):
            assert np.array_equal(got, fwd), (streams, call)
        assert np.array_equal(c.ntt(GOLD, W, a[0]), fwd[0]), (streams, "batch 1")
    finally:
        c.close()


def test_round_trip(ctx):
    for name in ("random", "low_zero", "high_zero"):
        a, fwd = refs(1)[name]
        assert np.array_equal(ctx.ntt(GOLD, W, fwd[0], inverse=True), a[0]), name
