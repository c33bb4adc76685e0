"""The fork and join of the two-stream batched Goldilocks NTT (ntt_launch.hip run_gl_passes):
the events that order the auxiliary stream against the caller's stream must keep the call an
ordinary stream operation. What a weaker release scope of those events, or a moved event,
could break is the ordering against the caller's own work before and after the call, and what
the host sees after a stream synchronisation; every case here runs with no synchronisation
between the producer of the input, the call and the consumer of the output.

n = 2^16 (the smallest size that runs the grouped schedule); batches 8 (two full groups of 4),
9 (three groups: the last, of 1, on the caller's stream, the auxiliary stream ends on a full
group) and 13 (four groups: the last, of 1, ends the auxiliary stream). Every expected value is
oracle.ntt_iter's, computed once for a pool of POOL polynomials that the calls draw from."""
import functools

import numpy as np
import pytest

import oracle
import pbf

pytestmark = pytest.mark.gpu
GOLD = pbf.GOLDILOCKS
N = 1 << 16
W = pow(7, (GOLD - 1) // N, GOLD)
POOL = 16
CALLS = 30
SETS = 3
SHIFT = 7
BATCHES = [8, 9, 13]


@functools.lru_cache(maxsize=1)
def pool():
    """Two seeded operand sets below 2^63 (so their XOR is a canonical element), the XOR, and
    the oracle's forward transform of each of its POOL polynomials; host arrays, never written."""
    pa = (oracle.splitmix_field(GOLD, 9100, POOL * N) >> np.uint64(1)).reshape(POOL, N)
    pb = (oracle.splitmix_field(GOLD, 9200, POOL * N) >> np.uint64(1)).reshape(POOL, N)
    x = pa ^ pb
    ref = np.stack([oracle.ntt_iter(GOLD, W, x[i]) for i in range(POOL)])
    for a in (pa, pb, x, ref):
        a.setflags(write=False)
    return pa, pb, x, ref


@functools.lru_cache(maxsize=1)
def dev_pool():
    import torch

    return tuple(torch.from_numpy(a.view(np.int64).copy()).cuda() for a in pool())


def picks(k, batch):
    """the pool polynomials of call k: a different selection every call"""
    return [(7 * k + i) % POOL for i in range(batch)]


def run_chain(ctx, batch, stream, call, expect, operands=None, from_host=False):
    """CALLS calls back to back on `stream` (the current torch stream), rotating SETS buffer
    pairs: a torch kernel writes the input (the XOR of two operand selections), `call` transforms
    it, a torch kernel copies the output away; one synchronisation at the end, then every copy
    is compared with `expect`'s rows. from_host: the input is instead written by an asynchronous
    copy from pinned host memory (the copy engine, not a kernel, is the producer; the rotating
    buffers hold an earlier call's input when it lands)."""
    import torch

    da, db, _, _ = dev_pool()
    if operands is not None:
        da, db = operands
    ins = [torch.empty(batch * N, dtype=torch.int64, device="cuda") for _ in range(SETS)]
    outs = [torch.empty(batch * N, dtype=torch.int64, device="cuda") for _ in range(SETS)]
    kept = [torch.empty(batch * N, dtype=torch.int64, device="cuda") for _ in range(CALLS)]
    idx = [torch.tensor(picks(k, batch), device="cuda") for k in range(CALLS)]
    if from_host:
        x = pool()[2]
        staged = [torch.from_numpy(x[picks(k, batch)].reshape(-1).view(np.int64)).pin_memory() for k in range(CALLS)]
    torch.cuda.synchronize()  # the set-up above ran on other streams
    for k in range(CALLS):
        i, o = ins[k % SETS], outs[k % SETS]
        if from_host:
            i.copy_(staged[k], non_blocking=True)
        else:
            torch.bitwise_xor(da[idx[k]], db[idx[k]], out=i.view(batch, N))
        call(ctx, i.data_ptr(), o.data_ptr(), batch, stream.cuda_stream)
        kept[k].copy_(o)
    stream.synchronize()
    for k in range(CALLS):
        assert torch.equal(kept[k].view(batch, N), expect[idx[k]]), f"call {k}"


def forward(ctx, d_in, d_out, batch, sp):
    ctx.ntt_batch_dev(GOLD, W, d_in, d_out, N, batch, stream=sp)


@pytest.mark.parametrize("batch", BATCHES)
def test_producer_and_consumer_on_the_stream(ctx, batch):
    import torch

    run_chain(ctx, batch, torch.cuda.current_stream(), forward, dev_pool()[3])


def test_input_copied_from_the_host_on_the_stream(ctx):
    """The caller's operation before each call is an asynchronous host-to-device copy: the
    auxiliary stream's kernels must read what the copy wrote, not lines an earlier call left in
    a cache (batch 9)."""
    import torch

    run_chain(ctx, 9, torch.cuda.current_stream(), forward, dev_pool()[3], from_host=True)


@pytest.mark.parametrize("batch", BATCHES)
def test_side_stream(ctx, batch):
    """The same chain on a torch stream that is not the default one."""
    import torch

    dev_pool()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run_chain(ctx, batch, side, forward, dev_pool()[3])


@pytest.mark.parametrize("batch", BATCHES)
def test_host_sees_the_output_after_a_stream_synchronisation(ctx, batch):
    """An asynchronous copy to pinned memory on the caller's stream, then a synchronisation of
    that stream only: the host reads the polynomials the auxiliary stream wrote too."""
    import torch

    _, _, dx, _ = dev_pool()
    ref = pool()[3]
    stream = torch.cuda.current_stream()
    host = torch.empty(batch * N, dtype=torch.int64).pin_memory()
    out = torch.empty(batch * N, dtype=torch.int64, device="cuda")
    for k in range(3):
        idx = picks(k, batch)
        d_in = dx[torch.tensor(idx, device="cuda")].contiguous()
        forward(ctx, d_in.data_ptr(), out.data_ptr(), batch, stream.cuda_stream)
        host.copy_(out, non_blocking=True)
        stream.synchronize()
        assert np.array_equal(host.numpy().view(np.uint64).reshape(batch, N), ref[idx]), f"call {k}"


def test_inverse_in_the_chain(ctx):
    """Inverse calls on batch 9: the producer writes forward transforms (the XOR of two masked
    operand sets), the expected output is the oracle's inverse of each."""
    import torch

    _, _, x, ref = pool()
    mask = oracle.splitmix_field(GOLD, 9300, POOL * N).reshape(POOL, N)
    ops = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (ref ^ mask, mask))
    back = np.stack([oracle.ntt_iter(GOLD, W, ref[i], inverse=True) for i in range(POOL)])
    assert np.array_equal(back, x)  # the oracle's own round trip
    expect = torch.from_numpy(back.view(np.int64)).cuda()

    def inverse(c, d_in, d_out, batch, sp):
        c.ntt_batch_dev(GOLD, W, d_in, d_out, N, batch, inverse=True, stream=sp)

    run_chain(ctx, 9, torch.cuda.current_stream(), inverse, expect, operands=ops)


def test_fused_coset_forward_in_the_chain(ctx):
    """The fused coset forward transform (pbf_ntt_u64_coset_batch_dev) on batch 9: expected
    oracle.ntt_iter of x[j] * shift^j."""
    import torch

    x = pool()[2]
    pw, s = [], 1
    for _ in range(N):
        pw.append(s)
        s = s * SHIFT % GOLD
    scaled = np.array([[int(v) * p % GOLD for v, p in zip(row, pw)] for row in x], dtype=np.uint64)
    expect = torch.from_numpy(np.stack([oracle.ntt_iter(GOLD, W, r) for r in scaled]).view(np.int64)).cuda()

    def coset(c, d_in, d_out, batch, sp):
        c.ntt_coset_batch_dev(GOLD, W, SHIFT, d_in, N, d_out, N, batch, stream=sp)

    run_chain(ctx, 9, torch.cuda.current_stream(), coset, expect)


@pytest.mark.parametrize("batch", BATCHES)
def test_schedule_options_give_identical_bytes(batch):
    """ntt.streams 1, 2 and 3 with ntt.group 2 and 4: the oracle's bytes from every schedule
    (3 streams over the two groups of batch 8 leave one auxiliary stream without a group)."""
    import torch

    _, _, dx, dref = dev_pool()
    idx = torch.tensor(picks(1, batch), device="cuda")
    d_in = dx[idx].contiguous()
    stream = torch.cuda.current_stream()
    for streams in (1, 2, 3):
        for group in (2, 4):
            c = pbf.Context(0, options={"ntt.streams": str(streams), "ntt.group": str(group)})
            try:
                out = torch.empty_like(d_in)
                for _ in range(2):  # the second call reuses the context's streams and events
                    out.zero_()
                    c.ntt_batch_dev(GOLD, W, d_in.data_ptr(), out.data_ptr(), N, batch, stream=stream.cuda_stream)
                    kept = out.clone()
                    stream.synchronize()
                    assert torch.equal(kept, dref[idx]), (streams, group)
            finally:
                c.close()
