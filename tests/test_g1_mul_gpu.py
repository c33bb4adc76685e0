"""The pointwise G1 product (csrc/g1_mul.hip, pbf_g1_bn254_mul*): out_i = [k_i] P_i, bit-exact:
canonical affine output is unique, so every comparison is word for word.

Expected values: with P_i = [e_i]G from pbf_g1_bn254_mul_base_dev, [k_i e_i mod r]G from one more
call of it; and the oracle's g1_mul for 8 random pairs through the host form.

Boundaries of the implementation, each with a size below, at and above it: 64 lanes per workgroup
(n = 63, 64, 65 and 255, 256, 257 for several workgroups); the window table's tile of
2^g1ntt.tile_log products per launch, by default 2^14 (n = 2^14 - 1, 2^14, 2^14 + 1) and 64 with
the option at its minimum (the small sizes again, on a context of its own)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as F  # noqa: E402

pytestmark = pytest.mark.gpu
R, Q = F.R, F.Q
SMALL = [1, 63, 64, 65, 255, 256, 257]
TILE = [(1 << 14) - 1, 1 << 14, (1 << 14) + 1]
EINVAL = 1


class Dev:
    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch

    def scalars(self, ks):
        return self.torch.from_numpy(F.ints_to_limbs(ks).view(np.int64)).cuda()

    def mul_base(self, ks):
        """[k]G for each k as one int64 tensor of 8 words per point; 0 gives (0, 0)."""
        d = self.scalars(ks)
        out = self.torch.empty(8 * len(ks), dtype=self.torch.int64, device="cuda")
        self.ctx.g1_mul_base_dev(d.data_ptr(), out.data_ptr(), len(ks))
        self.torch.cuda.synchronize()
        return out

    def points(self, t):
        v = F.limbs_to_ints(t.cpu().numpy().view(np.uint64))
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def mul(self, ctx, d_pts, d_ks, n, in_place, side_stream=False):
        torch = self.torch
        out = d_pts.clone() if in_place else torch.full((8 * n,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        src = out if in_place else d_pts
        if side_stream:
            st = torch.cuda.Stream()
            ctx.g1_mul_dev(src.data_ptr(), d_ks.data_ptr(), out.data_ptr(), n, stream=st.cuda_stream)
            st.synchronize()
        else:
            ctx.g1_mul_dev(src.data_ptr(), d_ks.data_ptr(), out.data_ptr(), n)
            torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def dev(ctx):
    return Dev(ctx)


@pytest.fixture(scope="module")
def tiled_ctx():
    import pbf

    c = pbf.Context(0, options={"g1ntt.tile_log": "6"})
    yield c
    c.close()


_CASES = {}


def random_case(dev, n):
    """(points [e_i]G, scalars k_i, expected [k_i e_i]G) of one size, computed once."""
    if n not in _CASES:
        rng = random.Random(4000 + n)
        es = [rng.randrange(1, R) for _ in range(n)]
        ks = [rng.randrange(R) for _ in range(n)]
        _CASES[n] = (dev.mul_base(es), dev.scalars(ks), dev.mul_base([k * e % R for k, e in zip(ks, es)]))
    return _CASES[n]


def check(dev, ctx, n):
    d_pts, d_ks, want = random_case(dev, n)
    for in_place in (False, True):
        assert dev.torch.equal(dev.mul(ctx, d_pts, d_ks, n, in_place), want), (n, in_place)
    assert dev.torch.equal(dev.mul(ctx, d_pts, d_ks, n, False, side_stream=True), want), n


@pytest.mark.parametrize("n", SMALL)
def test_against_the_base_product(ctx, dev, n):
    check(dev, ctx, n)


@pytest.mark.parametrize("n", SMALL)
def test_small_tiles(tiled_ctx, dev, n):
    """Several launches over one window table (g1ntt.tile_log = 6: 64 products each)."""
    check(dev, tiled_ctx, n)


@pytest.mark.parametrize("n", TILE)
def test_at_the_default_tile(ctx, dev, n):
    check(dev, ctx, n)


def exit_cases(rng):
    """(e, k) pairs: every exit of the window product, shuffled so that the lanes of one wave
    take different ones."""
    special = [0, 1, 2, 15, 16, R - 1, 1 << 252]
    pairs = []
    for k in special:  # each special scalar on a random point and on the identity
        pairs += [(rng.randrange(1, R), k), (0, k)]
    pairs += [(0, rng.randrange(R)) for _ in range(5)]  # P = (0, 0), full-width scalars
    e = rng.randrange(1, R)
    pairs += [(e, rng.randrange(R)) for _ in range(6)]  # equal points, different scalars
    pairs += [(e, k) for k in special]
    pairs += [(rng.randrange(1, R), rng.randrange(R)) for _ in range(40)]
    pairs += [(1, rng.randrange(R)), (R - 1, rng.randrange(R)), (1, R - 1), (R - 1, R - 1)]  # G and -G
    rng.shuffle(pairs)
    twin = (rng.randrange(1, R), rng.randrange(R))  # the same (point, scalar) in neighbouring lanes
    pairs[10:10] = [twin] * 3
    pairs[70:70] = [(twin[0], 7)] * 2
    return pairs


@pytest.mark.parametrize("which", ["default", "tiled"])
def test_exits_mixed_in_one_launch(ctx, tiled_ctx, dev, which):
    c = ctx if which == "default" else tiled_ctx
    pairs = exit_cases(random.Random(99))
    n = len(pairs)
    assert 64 < n < 128  # two waves, the second partly filled
    es, ks = [p[0] for p in pairs], [p[1] for p in pairs]
    d_pts, d_ks = dev.mul_base(es), dev.scalars(ks)
    want = dev.mul_base([k * e % R for k, e in zip(ks, es)])
    for in_place in (False, True):
        got = dev.mul(c, d_pts, d_ks, n, in_place)
        assert dev.torch.equal(got, want), in_place
    pts, got = dev.points(d_pts), dev.points(got)
    for (e, k), p, g in zip(pairs, pts, got):
        if e == 0 or k == 0:
            assert g == (0, 0)
        elif k == 1:
            assert g == p
        elif k == R - 1:
            assert g == (p[0], Q - p[1])  # -P
    assert got[10] == got[11] == got[12]


def test_against_the_oracle(ctx):
    rng = random.Random(2020)
    pts = [F.g1_mul(F.G1_GEN, rng.randrange(1, 1 << 16)) for _ in range(8)]
    ks = [rng.randrange(R) for _ in range(8)]
    want = [F.g1_mul(p, k) for p, k in zip(pts, ks)]
    assert ctx.g1_mul(pts, ks) == [(0, 0) if w is None else w for w in want]
    assert ctx.g1_mul([(0, 0), pts[0]], [5, 0]) == [(0, 0), (0, 0)]


def test_errors(ctx, dev):
    import pbf

    lib, h = ctx.lib, ctx.h
    n = 8
    pts = dev.points(dev.mul_base(list(range(1, n + 1))))
    ks = list(range(3, n + 3))
    p64 = lambda x: pbf._ptr(x)  # noqa: E731
    a, k = pbf._g1_limbs(pts), pbf.ints_to_limbs(ks)
    out = np.zeros(8 * n, dtype=np.uint64)
    host = lambda pa, ka, o, nn: lib.pbf_g1_bn254_mul(h, pa, ka, o, nn)  # noqa: E731
    assert host(p64(a), p64(k), p64(out), 0) == EINVAL
    assert lib.pbf_g1_bn254_mul(None, p64(a), p64(k), p64(out), n) == EINVAL
    assert host(None, p64(k), p64(out), n) == EINVAL
    assert host(p64(a), None, p64(out), n) == EINVAL
    assert host(p64(a), p64(k), None, n) == EINVAL
    off = list(pts)
    off[5] = (pts[5][0], (pts[5][1] + 1) % Q)  # off the curve
    assert host(p64(pbf._g1_limbs(off)), p64(k), p64(out), n) == EINVAL
    big = list(pts)
    big[2] = (pts[2][0] + Q, pts[2][1])  # x + q is on the curve mod q, and not canonical
    assert big[2][0] < 1 << 256
    assert host(p64(pbf._g1_limbs(big)), p64(k), p64(out), n) == EINVAL
    for bad_k in (R, R + 5, (1 << 256) - 1):
        assert host(p64(a), p64(pbf.ints_to_limbs(ks[:3] + [bad_k] + ks[4:])), p64(out), n) == EINVAL
    # the device form: n = 0 and NULL
    d_pts, d_ks = dev.mul_base(list(range(1, n + 1))), dev.scalars(ks)
    d_out = dev.torch.full((8 * n,), -1, dtype=dev.torch.int64, device="cuda")
    dev.torch.cuda.synchronize()
    vp = ctypes.c_void_p
    devf = lambda p, s, o, nn: lib.pbf_g1_bn254_mul_dev(h, p, s, o, nn, None)  # noqa: E731
    assert devf(vp(d_pts.data_ptr()), vp(d_ks.data_ptr()), vp(d_out.data_ptr()), 0) == EINVAL
    assert devf(None, vp(d_ks.data_ptr()), vp(d_out.data_ptr()), n) == EINVAL
    assert devf(vp(d_pts.data_ptr()), None, vp(d_out.data_ptr()), n) == EINVAL
    assert devf(vp(d_pts.data_ptr()), vp(d_ks.data_ptr()), None, n) == EINVAL
    assert lib.pbf_g1_bn254_mul_dev(None, vp(d_pts.data_ptr()), vp(d_ks.data_ptr()), vp(d_out.data_ptr()), n,
                                    None) == EINVAL
    # nothing was written
    dev.torch.cuda.synchronize()
    assert not out.any() and bool((d_out == -1).all())
    # and the next good call works, in both forms
    want = dev.points(dev.mul_base([e * kk % R for e, kk in zip(range(1, n + 1), ks)]))
    assert ctx.g1_mul(pts, ks) == want
    assert devf(vp(d_pts.data_ptr()), vp(d_ks.data_ptr()), vp(d_out.data_ptr()), n) == 0
    dev.torch.cuda.synchronize()
    assert dev.points(d_out) == want
