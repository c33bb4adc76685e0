"""pbf_pointwise_mul_u64_dev and pbf_pointwise_mul_fr256_dev (include/pbf.h) against Python
integers: the C ABI's most direct route to the device products (Goldilocks::mul, Mod32::mul,
Fr::mul of csrc/field.hpp and fp256.hpp).

Operands are the pair sets of tests/field_device_inputs.py (every correction of the Goldilocks
reduction, both sides of the 256-bit select, the Barrett correction), repeated to the counts
1, 255, 256, 257 and 2^20 + 1 (one block short, full, one over; and more elements than the
4096 blocks of the u64 launch hold, so its grid-stride loop runs), with the output aliasing
either input, both inputs the same buffer, on a caller's stream and on the null stream.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import field_device_inputs as fdi  # noqa: E402
from field_device_inputs import FR, GOLD  # noqa: E402

pytestmark = pytest.mark.gpu
COUNTS = [1, 255, 256, 257, (1 << 20) + 1]
SENTINEL = 0x5A5A5A5A5A5A5A5A


def dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def sync():
    import torch

    torch.cuda.synchronize()


def u64_pairs(m):
    pairs = fdi.gl_pairs() if m == GOLD else fdi.mod32_pairs(m)
    a, b = (fdi.u64(v) for v in zip(*pairs))
    return a, b, fdi.u64([x * y % m for x, y in pairs])


@pytest.mark.parametrize("m", [GOLD] + fdi.MOD32_MODULI)
def test_pointwise_mul_counts(ctx, m):
    a, b, ref = u64_pairs(m)
    if m == GOLD:
        cases = fdi.count_cases((fdi.red96_case(*fdi.mul_red96_args(int(x), int(y))) for x, y in zip(a, b)),
                                fdi.RED96_CASES)
        assert all(cases[c] >= 3 for c in fdi.RED96_CASES), cases
    assert len(a) > 257 and len(a) % 256 != 0
    for count in COUNTS:
        d_a, d_b = dev(np.resize(a, count)), dev(np.resize(b, count))
        d_c = dev(np.full(count + 1, SENTINEL, dtype=np.uint64))
        sync()
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), count)
        sync()
        got = host(d_c)
        bad = np.nonzero(got[:count] != np.resize(ref, count))[0]
        assert bad.size == 0, "modulus %d, count %d: %d differ, first at %d" % (m, count, bad.size, bad[0])
        assert got[count] == SENTINEL, "count %d: wrote past the end" % count


@pytest.mark.parametrize("m", [GOLD, 3221225473, (1 << 32) - 5])
def test_pointwise_mul_aliasing_and_streams(ctx, m):
    import torch

    a, b, ref = u64_pairs(m)
    n = len(a)
    sq = fdi.u64([int(x) * int(x) % m for x in a])
    side = torch.cuda.Stream()
    for stream in (0, side.cuda_stream):
        d_a, d_b = dev(a), dev(b)
        sync()
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_b.data_ptr(), d_a.data_ptr(), n, stream=stream)  # c == a
        sync()
        assert np.array_equal(host(d_a), ref) and np.array_equal(host(d_b), b)
        d_a = dev(a)
        sync()
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_b.data_ptr(), d_b.data_ptr(), n, stream=stream)  # c == b
        sync()
        assert np.array_equal(host(d_b), ref) and np.array_equal(host(d_a), a)
        d_c = dev(np.zeros(n, dtype=np.uint64))
        sync()
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), n, stream=stream)  # a == b
        sync()
        assert np.array_equal(host(d_c), sq) and np.array_equal(host(d_a), a)
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_a.data_ptr(), d_a.data_ptr(), n, stream=stream)  # all three
        sync()
        assert np.array_equal(host(d_a), sq)


def test_pointwise_mul_count_zero_and_unsupported_moduli(ctx):
    import pbf

    a, b, _ = u64_pairs(GOLD)
    d_a, d_b = dev(a[:300]), dev(b[:300])
    d_c = dev(np.full(300, SENTINEL, dtype=np.uint64))
    sync()
    for m in [GOLD, 337]:
        ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), 0)
        ctx.pointwise_mul_dev(m, 0, 0, 0, 0)
    for m in [2, 65536, (1 << 32) - 2, (1 << 61) - 1, (1 << 32) + 15]:
        with pytest.raises(pbf.PbfError) as err:
            ctx.pointwise_mul_dev(m, d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), 300)
        assert err.value.code == pbf.PBF_EUNSUPPORTED, m
    sync()
    assert np.all(host(d_c) == SENTINEL)
    assert np.array_equal(host(d_a), a[:300]) and np.array_equal(host(d_b), b[:300])


# ---- BN254 Fr ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr_pairs():
    pairs = fdi.fp_pairs(FR)
    a, b = (fdi.u256(v) for v in zip(*pairs))
    return pairs, a, b, fdi.u256([x * y % FR for x, y in pairs])


def test_fr_pointwise_mul_counts(ctx, fr_pairs):
    pairs, a, b, ref = fr_pairs
    # both sides of the final select of each of the kernel's two products (to_mont(a), then by b)
    rm = [x * fdi.R256 % FR for x, _ in pairs]
    for taken in ([fdi.mont_unreduced(x, fdi.R256 * fdi.R256 % FR, FR) >= FR for x, _ in pairs],
                  [fdi.mont_unreduced(xm, y, FR) >= FR for xm, (_, y) in zip(rm, pairs)]):
        assert min(sum(taken), len(taken) - sum(taken)) >= 3  # to_mont's factor 2^512 mod r is small: t >= r is rare
    assert len(a) > 257 and len(a) % 256 != 0
    for count in COUNTS:
        d_a, d_b = dev(np.resize(a, (count, 4))), dev(np.resize(b, (count, 4)))
        d_c = dev(np.full((count + 1, 4), SENTINEL, dtype=np.uint64))
        sync()
        ctx.fr_pointwise_mul_dev(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), count)
        sync()
        got = host(d_c)
        bad = np.nonzero((got[:count] != np.resize(ref, (count, 4))).any(axis=1))[0]
        assert bad.size == 0, "count %d: %d differ, first at %d" % (count, bad.size, bad[0])
        assert np.all(got[count] == SENTINEL), "count %d: wrote past the end" % count


def test_fr_pointwise_mul_aliasing_streams_and_count_zero(ctx, fr_pairs):
    import torch

    pairs, a, b, ref = fr_pairs
    n = len(pairs)
    sq = fdi.u256([x * x % FR for x, _ in pairs])
    side = torch.cuda.Stream()
    for stream in (0, side.cuda_stream):
        d_a, d_b = dev(a), dev(b)
        sync()
        ctx.fr_pointwise_mul_dev(d_a.data_ptr(), d_b.data_ptr(), d_a.data_ptr(), n, stream=stream)  # c == a
        sync()
        assert np.array_equal(host(d_a), ref) and np.array_equal(host(d_b), b)
        d_a = dev(a)
        sync()
        ctx.fr_pointwise_mul_dev(d_a.data_ptr(), d_b.data_ptr(), d_b.data_ptr(), n, stream=stream)  # c == b
        sync()
        assert np.array_equal(host(d_b), ref) and np.array_equal(host(d_a), a)
        d_c = dev(np.full((n, 4), SENTINEL, dtype=np.uint64))
        sync()
        ctx.fr_pointwise_mul_dev(d_a.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), 0, stream=stream)
        ctx.fr_pointwise_mul_dev(0, 0, 0, 0, stream=stream)
        sync()
        assert np.all(host(d_c) == SENTINEL)
        ctx.fr_pointwise_mul_dev(d_a.data_ptr(), d_a.data_ptr(), d_c.data_ptr(), n, stream=stream)  # a == b
        sync()
        assert np.array_equal(host(d_c), sq) and np.array_equal(host(d_a), a)
