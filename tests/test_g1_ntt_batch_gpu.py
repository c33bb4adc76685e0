"""The batched NTT over BN254 G1 (csrc/g1_ntt.hip pbf_ntt_g1_bn254_batch*), bit-exact: `batch`
transforms of size n under one omega, transform b at in + 8*b*n.

Two yardsticks. The single transform Context.ntt_g1_dev on every slice (tests/test_g1_ntt_gpu.py
ties it to the oracle). Independent of it, linearity: inputs [a_j]G from pbf_g1_bn254_mul_base_dev
give [NTT(a)_i]G, the right side over integers mod r: every transform at n <= 64, and the first
two, a middle one and the last above that.

Boundaries of the batched kernels, each met below:
  * transforms smaller than a wave, so that a wave spans several (n = 2, 4, 32 under any batch);
  * a batch that is no power of two: the lane split divides by batch x groups (3, 5, 17, 65);
  * the lane mapping: one transform switches to group-major at half-width 64 (n >= 128); a batch
    stays position-major while batch x groups >= 64 (n = 128 x 65, 256 x 64: every stage; 256 x 5,
    512 x 5: the last stages fall back);
  * 64 lanes per workgroup and the load's 256 threads, inside and between transforms
    (n x batch = 64 x 5, 32 x 65, 128 x 3, ...);
  * launches: at the default tile 2^14, n = 2048 x 17 has 17,408 butterflies per stage, two launches,
    the second partial and starting inside transform 16; with g1ntt.tile_log = 6, (64, 5) runs
    160 butterflies as 64 + 64 + 32 and (256, 3) 384 as six launches, their boundaries inside and
    between transforms."""
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
EINVAL = 1
SMALL = [(n, b) for n in (1, 2, 4, 32, 64, 128, 256, 512) for b in (1, 2, 3, 5)]
WIDE = [(n, b) for n in (1, 2, 4, 32, 64) for b in (64, 65)] + [(128, 65), (256, 64)]


def ntt_int(ks, omega, inverse=False):
    return list(ks) if len(ks) == 1 else F.ntt(list(ks), omega, inverse=inverse)


class Dev:
    """Device helpers: [k]G on the device, points to and from tensors, the two forms of the call."""

    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch

    def mul_base(self, ks):
        d = self.torch.from_numpy(F.ints_to_limbs(ks).view(np.int64)).cuda()
        out = self.torch.empty(8 * len(ks), dtype=self.torch.int64, device="cuda")
        self.ctx.g1_mul_base_dev(d.data_ptr(), out.data_ptr(), len(ks))
        self.torch.cuda.synchronize()
        return out

    def points(self, t):
        v = F.limbs_to_ints(t.cpu().numpy().view(np.uint64))
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def batch(self, ctx, omega, d_in, n, batch, inverse, in_place=False, side_stream=False):
        torch = self.torch
        out = d_in.clone() if in_place else torch.full((8 * n * batch,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream() if side_stream else None
        ctx.ntt_g1_batch_dev(omega, out.data_ptr() if in_place else d_in.data_ptr(), out.data_ptr(), n, batch,
                             inverse=inverse, stream=st.cuda_stream if st else 0)
        if st:
            st.synchronize()
        torch.cuda.synchronize()
        return out

    def singles(self, omega, d_in, n, batch, inverse):
        """The first yardstick: one call of the single transform per slice."""
        out = self.torch.full((8 * n * batch,), -1, dtype=self.torch.int64, device="cuda")
        self.torch.cuda.synchronize()
        for b in range(batch):
            self.ctx.ntt_g1_dev(omega, d_in.data_ptr() + 64 * b * n, out.data_ptr() + 64 * b * n, n, inverse=inverse)
        self.torch.cuda.synchronize()
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


def sampled(n, batch):
    """The transforms the second yardstick covers: all at n <= 64, else four with the last."""
    return list(range(batch)) if n <= 64 else sorted({0, 1, batch // 2, batch - 1} & set(range(batch)))


def check_shape(dev, ctx, n, batch, ks=None, seed=0, **kw):
    """Forward and inverse against both yardsticks, and the round trip; returns the forward result."""
    torch = dev.torch
    rng = random.Random(10007 * n + batch + seed)
    ks = ks or [rng.randrange(R) for _ in range(n * batch)]
    omega = F.root_of_unity(n) if n > 1 else 1
    d_in = dev.mul_base(ks)
    fwd = None
    for inverse in (False, True):
        got = dev.batch(ctx, omega, d_in, n, batch, inverse, **kw)
        assert torch.equal(got, dev.singles(omega, d_in, n, batch, inverse)), (n, batch, inverse)
        bs = sampled(n, batch)
        want = dev.mul_base([v for b in bs for v in ntt_int(ks[b * n:(b + 1) * n], omega, inverse)])
        assert torch.equal(got.view(batch, 8 * n)[bs], want.view(len(bs), 8 * n)), (n, batch, inverse)
        if not inverse:
            fwd = got
    assert torch.equal(dev.batch(ctx, omega, fwd, n, batch, True, **kw), d_in), (n, batch)  # inverse(forward(x)) == x
    return fwd


@pytest.mark.parametrize("n,batch", SMALL + WIDE)
def test_shapes(ctx, dev, n, batch):
    check_shape(dev, ctx, n, batch)


def test_two_launches_per_stage(ctx, dev):
    """n = 2048 x 17: 17,408 butterflies per stage against 2^14 per launch."""
    check_shape(dev, ctx, 2048, 17)


@pytest.mark.parametrize("n,batch", [(64, 5), (256, 3)])
def test_small_tiles(tiled_ctx, dev, n, batch):
    """g1ntt.tile_log = 6: launch boundaries inside and between transforms."""
    check_shape(dev, tiled_ctx, n, batch)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (1, 2, 0)])
def test_group_law_exits_side_by_side(ctx, dev, order):
    """One transform all identities, one all the same point P (P + P in the first stage, then
    P + (-P), then identity operands), one random, at n = 32: the 48 butterflies of a stage are one
    wave, so the exits of add2 are taken by neighbouring lanes."""
    n, rng = 32, random.Random(32)
    a = rng.randrange(1, R)
    kinds = [[0] * n, [a] * n, [rng.randrange(R) for _ in range(n)]]
    ks = [v for i in order for v in kinds[i]]
    fwd = check_shape(dev, ctx, n, 3, ks=ks)
    rows = fwd.view(3, 8 * n)
    zero, same = order.index(0), order.index(1)
    assert not bool(rows[zero].any())
    assert bool(rows[same][:8].any()) and not bool(rows[same][8:].any())  # [32 a]G, then identities


def test_in_place_and_side_stream(ctx, dev):
    for n, batch in ((32, 3), (128, 5)):
        ref = check_shape(dev, ctx, n, batch, seed=5)
        assert dev.torch.equal(check_shape(dev, ctx, n, batch, seed=5, in_place=True), ref)
        assert dev.torch.equal(check_shape(dev, ctx, n, batch, seed=5, side_stream=True), ref)


def test_host_form(ctx, dev):
    import pbf

    n, batch, rng = 8, 3, random.Random(8)
    ks = [rng.randrange(R) for _ in range(n * batch)]
    ks[5] = ks[n] = 0
    omega = F.root_of_unity(n)
    d_in = dev.mul_base(ks)
    pts = dev.points(d_in)
    for inverse in (False, True):
        want = dev.points(dev.batch(ctx, omega, d_in, n, batch, inverse))
        assert ctx.ntt_g1_batch(omega, pts, n, inverse=inverse) == want
        assert want == [p for b in range(batch) for p in ctx.ntt_g1(omega, pts[b * n:(b + 1) * n], inverse=inverse)]
    assert ctx.ntt_g1_batch(1, pts[:3], 1) == pts[:3]
    # a point off the curve in the last transform: PBF_EINVAL, output untouched
    off = list(pts)
    off[n * batch - 2] = (off[-2][0], (off[-2][1] + 1) % Q)
    out = np.zeros(8 * n * batch, dtype=np.uint64)
    w = pbf._ptr(pbf.ints_to_limbs([omega]))
    assert ctx.lib.pbf_ntt_g1_bn254_batch(ctx.h, w, pbf._ptr(pbf._g1_limbs(off)), pbf._ptr(out), n, batch, 0) == EINVAL
    assert not out.any()
    assert ctx.lib.pbf_ntt_g1_bn254_batch(ctx.h, w, pbf._ptr(pbf._g1_limbs(pts)), pbf._ptr(out), n, batch, 0) == 0
    assert out.any()


def test_errors(ctx, dev):
    import pbf

    lib, h = ctx.lib, ctx.h
    n, batch = 8, 3
    omega = F.root_of_unity(n)
    d_in = dev.mul_base(list(range(1, n * batch + 1)))
    a = pbf._g1_limbs(dev.points(d_in))
    out = np.zeros(8 * n * batch, dtype=np.uint64)
    d_out = dev.torch.full((8 * n * batch,), -1, dtype=dev.torch.int64, device="cuda")
    dev.torch.cuda.synchronize()
    vp = ctypes.c_void_p
    w = lambda v: pbf._ptr(pbf.ints_to_limbs([v]))  # noqa: E731

    def host(om=omega, arr=a, o=out, nn=n, b=batch, ctxh=h):
        p = lambda v: None if v is None else pbf._ptr(v)  # noqa: E731
        return lib.pbf_ntt_g1_bn254_batch(ctxh, None if om is None else w(om), p(arr), p(o), nn, b, 0)

    def devf(om=omega, i=d_in.data_ptr(), o=d_out.data_ptr(), nn=n, b=batch, ctxh=h):
        return lib.pbf_ntt_g1_bn254_batch_dev(ctxh, None if om is None else w(om), vp(i) if i else None,
                                              vp(o) if o else None, nn, b, 1, None)

    for nn in (0, 3, 6, 12, 1 << 29):
        assert host(nn=nn) == EINVAL and devf(nn=nn) == EINVAL, nn
    for om in (F.root_of_unity(n // 2), F.root_of_unity(2 * n), 0, 1, R, R + omega):
        assert host(om=om) == EINVAL and devf(om=om) == EINVAL, om
    assert host(b=0) == EINVAL and devf(b=0) == EINVAL
    # the product limit: n * batch = 2^28 + n, and twice the largest single transform
    assert host(b=(1 << 25) + 1) == EINVAL and devf(b=(1 << 25) + 1) == EINVAL
    big = F.root_of_unity(1 << 28)
    assert host(om=big, nn=1 << 28, b=2) == EINVAL and devf(om=big, nn=1 << 28, b=2) == EINVAL
    assert host(b=1 << 62) == EINVAL and devf(b=1 << 62) == EINVAL
    assert host(om=None) == EINVAL and host(arr=None) == EINVAL and host(o=None) == EINVAL and host(ctxh=None) == EINVAL
    assert devf(om=None) == EINVAL and devf(i=0) == EINVAL and devf(o=0) == EINVAL and devf(ctxh=None) == EINVAL
    # nothing was enqueued or written
    dev.torch.cuda.synchronize()
    assert not out.any() and bool((d_out == -1).all())
    # and the same arguments, valid, succeed
    assert host() == 0 and devf() == 0
    dev.torch.cuda.synchronize()
    assert out.any() and not bool((d_out == -1).all())
