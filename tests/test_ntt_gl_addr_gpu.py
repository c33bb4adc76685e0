"""The global addresses of the two "10,10" pass kernels of the 2^20 default plan (ntt_gl.hpp
SP 2): every load and store takes a wave-uniform 64-bit base (pointer, polynomial, tile and the
stride of the access) plus one 32-bit byte offset per lane. 2^20 is the only size that runs these
kernels, so every case is at 2^20 and the batches are small.

What such addressing can get wrong and the case that shows it:
  - a base assumed aligned to more than 8 B: input and output as views that start 1 and 4097
    elements into larger allocations;
  - an access outside the polynomials: 1024 sentinel words before and after the output and after
    the input, unchanged after batches 1, 9 and 17 (groups 8 + 8 + 1);
  - a polynomial's base folded into a 32-bit offset: batch 514 in one launch (ntt.group 0), where
    polynomials 511, 512 and 513 lie across the 4 GiB byte offset of input, intermediate and
    output, and the same batch under the default groups of 8 (about 13 GB of device memory);
  - a group or stream combination: ntt.streams 1 and 2 x ntt.group 4 and 8 at batch 17.

The reference is oracle.ntt_gl_par on 8 distinct random polynomials, computed once; larger batches
repeat those 8."""
import numpy as np
import pytest

import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
LOGN = 20
N = 1 << LOGN
W = pow(7, (GOLD - 1) // N, GOLD)
POLYS = 8
GUARD = 1024
SENTINEL = 0x5AA5C33C0FF0A55A  # below 2^63: the same bits as int64 and as uint64
BIG = 514  # 512 polynomials of 8 MiB are 4 GiB: 511 ends there, 512 and 513 lie past it

_REF = []


def ref():
    """(inputs [8][N], forward transforms [8][N]) by the oracle, computed once, read-only"""
    if not _REF:
        rng = np.random.default_rng(1100)
        a = rng.integers(0, GOLD, (POLYS, N), dtype=np.uint64)
        fwd = oracle.ntt_gl_par(W, a.reshape(-1), batch=POLYS).reshape(POLYS, N)
        assert np.array_equal(fwd[0], oracle.ntt_iter(GOLD, W, a[0]))  # the two oracles, once
        a.setflags(write=False)
        fwd.setflags(write=False)
        _REF.extend((a, fwd))
    return _REF


def repeated(x, batch):
    """[batch][N]: polynomial i is x[i mod 8]"""
    return x[np.arange(batch) % POLYS]


def forward_views(c, batch, in_skip, out_skip, in_tail=0, out_tail=0, fill=0):
    """One batched forward transform of the repeated inputs from a view that starts in_skip
    elements into its allocation to one that starts out_skip elements into its own, in_tail and
    out_tail elements after them; both allocations hold `fill` everywhere else. Returns the two
    whole allocations on the host as uint64."""
    import torch

    a = repeated(ref()[0], batch).reshape(-1)
    d_in = torch.full((in_skip + batch * N + in_tail,), fill, dtype=torch.int64, device="cuda")
    d_out = torch.full((out_skip + batch * N + out_tail,), fill, dtype=torch.int64, device="cuda")
    d_in[in_skip:in_skip + batch * N] = torch.from_numpy(a.view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    c.ntt_batch_dev(GOLD, W, d_in.data_ptr() + 8 * in_skip, d_out.data_ptr() + 8 * out_skip, N, batch, stream=stream)
    torch.cuda.synchronize()
    return d_in.cpu().numpy().view(np.uint64), d_out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("skips", [(1, 4097), (4097, 1)])
def test_unaligned_bases(ctx, batch, skips):
    """bases 8-B aligned, not 16-B or 128-B aligned: 1 and 4097 elements into the allocations"""
    in_skip, out_skip = skips
    _, out = forward_views(ctx, batch, in_skip, out_skip)
    want = repeated(ref()[1], batch)
    got = out[out_skip:].reshape(batch, N)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (batch, skips, bad.tolist())


@pytest.mark.parametrize("batch", [1, 9, 17])
def test_guards(ctx, batch):
    """1024 sentinel words before and after the output and after the input stay as they were"""
    inp, out = forward_views(ctx, batch, 0, GUARD, in_tail=GUARD, out_tail=GUARD, fill=SENTINEL)
    want = repeated(ref()[1], batch)
    got = out[GUARD:GUARD + batch * N].reshape(batch, N)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (batch, bad.tolist())
    s = np.uint64(SENTINEL)
    assert (out[:GUARD] == s).all(), "words before the output"
    assert (out[GUARD + batch * N:] == s).all(), "words after the output"
    assert (inp[batch * N:] == s).all(), "words after the input"
    assert np.array_equal(inp[:batch * N].reshape(batch, N), repeated(ref()[0], batch)), "the input itself"


@pytest.mark.parametrize("group", ["0", None])
def test_4gib_boundary(group):
    """Batch 514: ntt.group 0 runs the whole batch as one launch per pass (65,792 workgroups, a
    tile-major intermediate of 514 x 8 MiB), the default takes groups of 8. The first 8 outputs
    against the oracle, every other output against its counterpart among the first 8."""
    import torch

    a, fwd = ref()
    c = pbf.Context(0, options={"ntt.group": group} if group is not None else None)
    try:
        d8 = torch.from_numpy(np.array(a).view(np.int64)).cuda()
        d_in = d8.repeat(BIG // POLYS + 1, 1)[:BIG].contiguous()
        assert d_in.shape == (BIG, N) and d_in.numel() * 8 > 1 << 32
        d_out = torch.zeros_like(d_in)
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        c.ntt_batch_dev(GOLD, W, d_in.data_ptr(), d_out.data_ptr(), N, BIG, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_out[:POLYS].cpu().numpy().view(np.uint64), fwd), "first 8 against the oracle"
        bad = [i for i in range(POLYS, BIG, POLYS) if not torch.equal(d_out[i:i + POLYS], d_out[:min(POLYS, BIG - i)])]
        assert not bad, ("outputs that differ from their counterparts, first polynomial of each 8", bad)
        assert torch.equal(d_in[:POLYS], d8) and torch.equal(d_in[BIG - 2:], d8[:2]), "the input itself"
    finally:
        c.close()
        d8 = d_in = d_out = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("streams", [1, 2])
def test_schedule_variants(streams, group):
    """batch 17 as 4 + 4 + 4 + 4 + 1 and 8 + 8 + 1 on one and two streams, two calls back to back"""
    import torch

    batch = 17
    a, want = repeated(ref()[0], batch), repeated(ref()[1], batch)
    c = pbf.Context(0, options={"ntt.group": str(group), "ntt.streams": str(streams)})
    try:
        d_in = torch.from_numpy(a.view(np.int64)).cuda()
        outs = [torch.zeros_like(d_in) for _ in range(2)]
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        for o in outs:
            c.ntt_batch_dev(GOLD, W, d_in.data_ptr(), o.data_ptr(), N, batch, stream=stream)
        torch.cuda.synchronize()
        for call, o in enumerate(outs):
            bad = np.flatnonzero((o.cpu().numpy().view(np.uint64) != want).any(axis=1))
            assert bad.size == 0, (streams, group, call, bad.tolist())
    finally:
        c.close()
