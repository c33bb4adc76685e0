"""Two-pass Goldilocks plans with a radix-2^10 pass: the specialised second-pass kernel of
plain forward plans (ntt_gl.hpp SP, selected in ntt_launch.hip run_gl_group), the stage-B
twiddle signs folded into the 16-point DFT (every pass kernel, dft_reg_signed) and the
per-stream scratch ring of the group schedule (run_gl_passes), bit-exact against the oracle.

Plans: 2^16 as "10,6" (radix 2^10 first: the generic kernel) and "6,10" (specialised second
pass, log_ns from the arguments): the smallest size with a radix-2^10 pass; 2^20 as "10,10"
(specialised second pass with log_ns = 10 compiled in). The inverse of each runs the generic
kernels. Inputs: carry / borrow edge values, all p-1, all 2^32-1, and unit impulses (every
output is then one twiddle power, so a sign applied to the wrong butterfly output shows)."""
import numpy as np
import pytest

import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
EDGE_GL = [0, 1, 2, GOLD - 1, GOLD - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) - 1,
           GOLD - (1 << 32), GOLD - (1 << 32) + 1, (1 << 64) - (1 << 33), 0xFFFFFFFE00000001, 0x00000000FFFFFFFF,
           0x7FFFFFFF80000000]  # the values of tests/test_ntt_gpu.py
PLANS = [(16, "10,6"), (16, "6,10"), (20, "10,10")]


def root(n):
    return pow(7, (GOLD - 1) // n, GOLD)


def inputs(logn):
    n = 1 << logn
    rng = np.random.default_rng(2000 + logn)
    ins = {"edge": np.array(EDGE_GL, dtype=np.uint64)[rng.integers(0, len(EDGE_GL), n)],
           "all_p_minus_1": np.full(n, GOLD - 1, dtype=np.uint64),
           "all_2p32_minus_1": np.full(n, (1 << 32) - 1, dtype=np.uint64)}
    for pos in (0, 1, 63, 64, 1023, n - 1):
        a = np.zeros(n, dtype=np.uint64)
        a[pos] = 1
        ins[f"impulse_{pos}"] = a
    return ins


_REFS = {}


def refs(logn):
    """name -> (input, forward, inverse) by oracle.ntt_iter, computed once per size"""
    if logn not in _REFS:
        w = root(1 << logn)
        _REFS[logn] = {k: (a, oracle.ntt_iter(GOLD, w, a), oracle.ntt_iter(GOLD, w, a, inverse=True))
                       for k, a in inputs(logn).items()}
        for v in _REFS[logn].values():
            for x in v:
                x.setflags(write=False)
    return _REFS[logn]


@pytest.mark.parametrize("logn,passes", PLANS)
def test_two_pass_plans_vs_oracle(logn, passes):
    c = pbf.Context(0, options={"ntt.passes": passes})
    try:
        w = root(1 << logn)
        for name, (a, fwd, inv) in refs(logn).items():
            got = c.ntt(GOLD, w, a)
            assert np.array_equal(got, fwd), (name, "forward")
            assert np.array_equal(c.ntt(GOLD, w, a, inverse=True), inv), (name, "inverse")
            assert np.array_equal(c.ntt(GOLD, w, got, inverse=True), a), (name, "round trip")
    finally:
        c.close()


@pytest.mark.parametrize("passes", ["10,6", "6,10"])
@pytest.mark.parametrize("batch", [8, 9])
def test_batches_match_single(passes, batch):
    """Batches 8 (two full groups, one per stream) and 9 (a ragged third group that reuses the
    first stream's scratch slot) against the same polynomials transformed one by one; two
    batched calls back to back, so a slot reused before its reader has finished shows."""
    import torch

    c = pbf.Context(0, options={"ntt.passes": passes})
    try:
        n = 1 << 16
        w = root(n)
        host = [np.stack([oracle.splitmix_field(GOLD, 900 + 16 * s + i, n) for i in range(batch)]) for s in range(2)]
        for inverse in (False, True):
            d_in = [torch.from_numpy(h.view(np.int64)).cuda() for h in host]
            d_out = [torch.empty_like(d) for d in d_in]
            stream = torch.cuda.current_stream().cuda_stream
            for s in range(2):
                c.ntt_batch_dev(GOLD, w, d_in[s].data_ptr(), d_out[s].data_ptr(), n, batch, inverse=inverse,
                                stream=stream)
            torch.cuda.synchronize()
            for s in range(2):
                got = d_out[s].cpu().numpy().view(np.uint64)
                for i in range(batch):
                    assert np.array_equal(got[i], c.ntt(GOLD, w, host[s][i], inverse=inverse)), (inverse, s, i)
    finally:
        c.close()
