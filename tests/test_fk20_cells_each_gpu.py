"""The cell proofs of every polynomial of a batch in one call (csrc/kzg_cells.hip
pbf_kzg_open_cells_each_bn254*), bit-exact: out_w[b*k + i] = W_i of p_b.

Two yardsticks. pbf_kzg_open_cells_bn254_dev on polynomial b alone under weight 1: every cell and
every value of every polynomial, torch.equal (tests/test_fk20_cells_gpu.py ties that call to the
trapdoor and the verifier). Independent of it, the trapdoor S of the test SRS: W_i = [q_i(S)]G for
the quotient of p_b by x^l - c_i from long division (tests/fk20_cells_expect.py), through
pbf_g1_bn254_mul_base_dev: every cell at n <= 64, and cells 0, 1, k/2 and k-1 above.

The scheme's own boundary: the batch x 2n products run as one vector in launches of
2^g1ntt.tile_log. Every shape with 2n below the tile has polynomials sharing a launch. With the
option at 6, (16, 4) x 3 is 96 products: polynomials 0 and 1 in one launch, polynomial 2 in a
partial one; (2^10, .) x 3 splits every polynomial over 32 launches. At the default 2^14,
(2^12, 64) x 3 is a full launch of two polynomials and a partial one of the third, and
(2^13, 64) x 2 one full launch each. Sizes are powers of two, so a launch never holds parts of two
polynomials without holding one of them whole."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import fk20_cells_expect as C  # noqa: E402
import fk20_expect as K  # noqa: E402

pytestmark = pytest.mark.gpu
R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R  # the trapdoor
M = 1 << 13  # device SRS: M + 1 points
EINVAL = 1


def omega2_of(n):
    return F.root_of_unity(2 * n)


def omega_of(n):
    return pow(omega2_of(n), 2, R)


class World:
    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch
        self.d_srs = torch.empty(8 * (M + 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.srs_create_dev(S, M, self.d_srs.data_ptr())
        torch.cuda.synchronize()
        self._xext, self._g2 = {}, {}

    def host_srs(self, m):
        return self.points(self.d_srs[:8 * m])

    def g2s(self, l):
        """[G2, [s^l]G2], the l-th power from the trapdoor."""
        if l not in self._g2:
            self._g2[l] = [B.G2_GEN, self.ctx.g2_bn254_mul([B.G2_GEN], [pow(S, l, R)])[0]]
        return self._g2[l]

    def mul_base(self, ks):
        d = self.torch.from_numpy(F.ints_to_limbs(ks).view(np.int64)).cuda()
        out = self.torch.empty(8 * len(ks), dtype=self.torch.int64, device="cuda")
        self.ctx.g1_mul_base_dev(d.data_ptr(), out.data_ptr(), len(ks))
        self.torch.cuda.synchronize()
        return out

    def points(self, t):
        v = F.limbs_to_ints(t.cpu().numpy().view(np.uint64))
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def xext(self, ctx, n, l):
        """The setup of (n, l) on the device, once per (context, n, l)."""
        key = (id(ctx), n, l)
        if key not in self._xext:
            out = self.torch.full((16 * n,), -1, dtype=self.torch.int64, device="cuda")
            self.torch.cuda.synchronize()
            ctx.kzg_cells_setup_dev(self.d_srs.data_ptr(), M + 1, omega2_of(n), n, l, out.data_ptr())
            self.torch.cuda.synchronize()
            self._xext[key] = out
        return self._xext[key]

    def dev_polys(self, polys, pitch, seed=1):
        """The polynomials (lists of one length) at `pitch`, the gaps filled with random values."""
        a = F.random_limbs(len(polys) * pitch, seed)
        for b, p in enumerate(polys):
            a[4 * b * pitch:4 * (b * pitch + len(p))] = F.ints_to_limbs(p)
        return self.torch.from_numpy(a.view(np.int64)).cuda()

    def open_each(self, ctx, n, l, d_p, ln, pitch, batch, with_y=True, side_stream=False):
        """(d_y or None, d_w) of the call under test; a skipped d_y is checked untouched."""
        torch = self.torch
        d_y = torch.full((4 * batch * n,), -1, dtype=torch.int64, device="cuda")
        d_w = torch.full((8 * batch * (n // l),), -1, dtype=torch.int64, device="cuda")
        x = self.xext(ctx, n, l)
        torch.cuda.synchronize()
        st = torch.cuda.Stream() if side_stream else None
        ctx.kzg_open_cells_each_dev(x.data_ptr(), n, l, omega2_of(n), d_p.data_ptr(), ln, pitch, batch,
                                    d_y.data_ptr() if with_y else 0, d_w.data_ptr(), stream=st.cuda_stream if st else 0)
        if st:
            st.synchronize()
        torch.cuda.synchronize()
        if not with_y:
            assert bool((d_y == -1).all())
        return (d_y if with_y else None), d_w

    def open_single(self, n, l, d_p, ln, pitch, b):
        """The first yardstick: the weighted call on polynomial b alone, weight 1 (the default context)."""
        torch = self.torch
        d_y = torch.full((4 * n,), -1, dtype=torch.int64, device="cuda")
        d_w = torch.full((8 * (n // l),), -1, dtype=torch.int64, device="cuda")
        x = self.xext(self.ctx, n, l)
        torch.cuda.synchronize()
        self.ctx.kzg_open_cells_dev(x.data_ptr(), n, l, omega2_of(n), d_p.data_ptr() + 32 * b * pitch, ln, ln, 1, [1],
                                    d_y.data_ptr(), d_w.data_ptr())
        torch.cuda.synchronize()
        return d_y, d_w


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


@pytest.fixture(scope="module")
def tiled_ctx():
    import pbf

    c = pbf.Context(0, options={"g1ntt.tile_log": "6"})
    yield c
    c.close()


def sample_cells(n, k):
    """Every cell at n <= 64, else the first two, the middle and the last."""
    return list(range(k)) if n <= 64 else sorted({0, 1, k // 2, k - 1})


def expect_w(p, n, l, cells):
    """The scalars of W_i for i in cells, by long division of p by x^l - c_i."""
    omega, p = omega_of(n), K.padded(p, n)
    return [F.poly_eval(C.divide(p, l, pow(omega, i * l, R))[0] or [0], S) for i in cells]


def random_polys(rng, batch, ln):
    return [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]


def check(world, ctx, n, l, polys, pitch=None, **kw):
    """One call against both yardsticks, each polynomial on its own; returns (d_y, d_w)."""
    torch = world.torch
    ln, batch, k = len(polys[0]), len(polys), n // l
    pitch = pitch or ln
    d_p = world.dev_polys(polys, pitch)
    d_y, d_w = world.open_each(ctx, n, l, d_p, ln, pitch, batch, **kw)
    cells = sample_cells(n, k)
    for b, p in enumerate(polys):
        one_y, one_w = world.open_single(n, l, d_p, ln, pitch, b)
        assert torch.equal(d_w[8 * b * k:8 * (b + 1) * k], one_w), (n, l, b)
        if d_y is not None:
            assert torch.equal(d_y[4 * b * n:4 * (b + 1) * n], one_y), (n, l, b)
    want = world.mul_base([v for p in polys for v in expect_w(p, n, l, cells)])
    assert torch.equal(d_w.view(batch, k, 8)[:, cells], want.view(batch, len(cells), 8)), (n, l)
    if d_y is not None and n <= 64:
        v = F.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
        got = [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)]
        assert got == [C.cell_values(p, n, l, omega_of(n)) for p in polys]
    return d_y, d_w


def check_random(world, ctx, n, l, batch, ln, seed, **kw):
    polys = random_polys(random.Random(seed), batch, ln)
    return (polys,) + check(world, ctx, n, l, polys, **kw)


# ---------------------------------------------------------------- every shape up to n = 64
POW2 = [1, 2, 4, 8, 16, 32, 64]
SHAPES = [(n, l) for n in POW2 for l in POW2 if l <= n]


@pytest.mark.parametrize("n,l", SHAPES)
def test_every_shape(ctx, world, n, l):
    polys, d_y, d_w = check_random(world, ctx, n, l, 3, n, 100 * n + l)
    if l == n:  # one cell: the whole domain; the quotient is zero
        assert not bool(d_w.any())
    if l == 1:  # every opening of every polynomial: open_all per polynomial, weight 1
        torch = world.torch
        d_p = world.dev_polys(polys, n)
        x = world.xext(ctx, n, 1)
        for b in range(3):
            y20 = torch.full((4 * n,), -1, dtype=torch.int64, device="cuda")
            w20 = torch.full((8 * n,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.kzg_open_all_dev(x.data_ptr(), n, omega2_of(n), d_p.data_ptr() + 32 * b * n, n, n, 1, [1], y20.data_ptr(),
                                 w20.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(d_w[8 * b * n:8 * (b + 1) * n], w20) and torch.equal(d_y[4 * b * n:4 * (b + 1) * n], y20)


# ---------------------------------------------------------------- boundaries of transforms and products
@pytest.mark.parametrize("n,l,batch", [(512, 2, 3), (1 << 11, 64, 2), (1 << 12, 64, 3), (1 << 13, 64, 2)])
def test_transform_and_launch_boundaries(ctx, world, n, l, batch):
    check_random(world, ctx, n, l, batch, n, 7 * n + l)


@pytest.mark.parametrize("n,l,batch", [(16, 4, 3), (16, 4, 5), (1 << 10, 4, 3), (1 << 10, 64, 3)])
def test_small_tiles(tiled_ctx, world, n, l, batch):
    """g1ntt.tile_log = 6: see the head of the file."""
    check_random(world, tiled_ctx, n, l, batch, n, 66 + l + batch)


# ---------------------------------------------------------------- unlike members of one batch
def test_unlike_members(ctx, world):
    """Random polynomials around: the zero polynomial in the middle; one of true degree below l;
    one with p_(2u) = S p_(2u+1) (slabs r, r + 1 have equal products: the sum meets P + P) and one
    with p_(2u) = -S p_(2u+1) (they cancel: P + (-P), then the identity as an operand)."""
    n, l, rng = 64, 8, random.Random(648)
    k = n // l
    odd = [rng.randrange(1, R) for _ in range(n // 2)]
    equal = [v for o in odd for v in (S * o % R, o)]
    opposite = [v for o in odd for v in ((R - S) * o % R, o)]
    low = [rng.randrange(1, R) for _ in range(l - 1)] + [0] * (n - l + 1)
    rnd = random_polys(rng, 4, n)
    polys = [rnd[0], equal, rnd[1], [0] * n, rnd[2], opposite, low, rnd[3]]
    d_y, d_w = check(world, ctx, n, l, polys)
    rows = d_w.view(len(polys), 8 * k)
    for b, p in enumerate(polys):
        assert bool(rows[b].any()) == (p not in ([0] * n, opposite, low)), b
    assert not bool(d_y[4 * 3 * n:4 * 4 * n].any())  # the values of the zero polynomial


# ---------------------------------------------------------------- lengths, pitch, batches, call forms
def test_lengths(ctx, world):
    n, l = 64, 8
    for ln in (1, l, l + 1, n - 1, n):
        _, _, d_w = check_random(world, ctx, n, l, 3, ln, 40 * n + ln)
        assert bool(d_w.any()) == (ln > l)  # degree below l: every quotient is zero


def test_pitch_and_without_y(ctx, world):
    n, l, ln = 64, 8, 61
    polys, _, d_w = check_random(world, ctx, n, l, 3, ln, 11)
    assert world.torch.equal(check(world, ctx, n, l, polys, pitch=ln + 5)[1], d_w)
    none, without = check(world, ctx, n, l, polys, with_y=False)
    assert none is None and world.torch.equal(without, d_w)
    assert world.torch.equal(check(world, ctx, n, l, polys, pitch=ln + 5, with_y=False)[1], d_w)


def test_side_stream(ctx, world):
    check_random(world, ctx, 64, 8, 3, 64, 12, side_stream=True)
    check_random(world, ctx, 512, 2, 2, 512, 13, side_stream=True)


@pytest.mark.parametrize("batch", [1, 70])
def test_batches(ctx, world, batch):
    check_random(world, ctx, 64, 8, batch, 64, 7 + batch)


def test_host_form(ctx, world):
    n, l, rng = 32, 4, random.Random(12)
    k = n // l
    polys = random_polys(rng, 3, n - 2)
    xext = world.points(world.xext(ctx, n, l))
    d_y, d_w = check(world, ctx, n, l, polys)
    v = F.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
    want_y = [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(3)]
    pts = world.points(d_w)
    want_w = [pts[b * k:(b + 1) * k] for b in range(3)]
    assert ctx.kzg_open_cells_each(xext, l, omega2_of(n), polys) == (want_y, want_w)
    assert ctx.kzg_open_cells_each(xext, l, omega2_of(n), polys, pitch=n + 1) == (want_y, want_w)
    assert ctx.kzg_open_cells_each(xext, l, omega2_of(n), polys, with_y=False) == (None, want_w)
    assert ctx.kzg_open_cells_each([(0, 0), (0, 0)], 1, R - 1, [[5], [6]]) == ([[[5]], [[6]]], [[(0, 0)], [(0, 0)]])


# ---------------------------------------------------------------- recover, prove, verify
@pytest.mark.parametrize("n,l", [(64, 8), (1024, 64)])
def test_recover_prove_verify(ctx, world, n, l):
    torch = world.torch
    k, batch, omega, rng = n // l, 3, omega_of(n), random.Random(n + l)
    ln = n // 2  # the 2x extension
    polys = random_polys(rng, batch, ln)
    d_p = world.dev_polys(polys, ln)
    commits = ctx.kzg_commit_dev(world.d_srs.data_ptr(), M + 1, d_p.data_ptr(), ln, ln, batch)
    d_y, d_w = world.open_each(ctx, n, l, d_p, ln, ln, batch)
    # a random half of the cells is dropped, the same for every polynomial
    keep = sorted(rng.sample(range(k), k // 2))
    idx = torch.tensor(keep, device="cuda")
    d_cells = d_y.view(batch, k, 4 * l)[:, idx].contiguous()
    d_rp = torch.full((4 * batch * ln,), -1, dtype=torch.int64, device="cuda")
    d_ry = torch.full((4 * batch * n,), -1, dtype=torch.int64, device="cuda")
    d_ok = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.kzg_recover_cells_dev(omega, n, l, ln, keep, d_cells.data_ptr(), batch, d_rp.data_ptr(), ln, d_ry.data_ptr(),
                              d_ok.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.tolist() == [1] * batch and torch.equal(d_rp, d_p) and torch.equal(d_ry, d_y)
    # the proofs of the recovered coefficients are the originals
    _, d_rw = world.open_each(ctx, n, l, d_rp, ln, ln, batch)
    assert torch.equal(d_rw, d_w)
    # and the verifier takes all 3k entries in one call
    ws = world.points(d_rw)
    v = F.limbs_to_ints(d_ry.cpu().numpy().view(np.uint64))
    entries = [(commits[b], i, v[(b * k + i) * l:(b * k + i + 1) * l], ws[b * k + i]) for b in range(batch) for i in range(k)]
    rhos = [rng.randrange(1, R) for _ in entries]
    g2s, srs = world.g2s(l), world.host_srs(l)
    assert ctx.kzg_verify_cells(g2s, srs, omega, n, l, entries, rhos)
    c, i, ys, w = entries[-1]
    bad_ys = list(ys)
    bad_ys[l - 1] = (bad_ys[l - 1] + 1) % R
    assert not ctx.kzg_verify_cells(g2s, srs, omega, n, l, entries[:-1] + [(c, i, bad_ys, w)], rhos)


# ---------------------------------------------------------------- errors
def test_errors(ctx, world):
    import pbf

    lib, h = ctx.lib, ctx.h
    n, l, ln, batch = 16, 4, 16, 2
    k = n // l
    vp = ctypes.c_void_p
    w = lambda v: pbf._ptr(pbf.ints_to_limbs([v]))  # noqa: E731
    w2 = omega2_of(n)
    x = world.xext(ctx, n, l)
    polys = random_polys(random.Random(1), batch, ln)
    d_p = world.dev_polys(polys, ln)
    d_y = world.torch.full((4 * batch * n,), -1, dtype=world.torch.int64, device="cuda")
    d_w = world.torch.full((8 * batch * k,), -1, dtype=world.torch.int64, device="cuda")
    world.torch.cuda.synchronize()

    def opn(xx=vp(x.data_ptr()), nn=n, ll=l, om=w2, p=vp(d_p.data_ptr()), le=ln, pitch=ln, b=batch, y=vp(d_y.data_ptr()),
            ww=vp(d_w.data_ptr()), ctxh=h):
        return lib.pbf_kzg_open_cells_each_bn254_dev(ctxh, xx, nn, ll, w(om) if om is not None else None, p, le, pitch, b,
                                                     y, ww, None)

    # the host form, on the same arguments
    a = pbf.ints_to_limbs([c for p in polys for c in p])
    hx = pbf._g1_limbs(world.points(x))
    out_y = np.zeros(4 * batch * n, dtype=np.uint64)
    out_w = np.zeros(8 * batch * k, dtype=np.uint64)

    def host(nn=n, ll=l, om=w2, le=ln, pitch=ln, b=batch, xx=hx, p=a, ww=out_w):
        q = lambda v: None if v is None else pbf._ptr(v)  # noqa: E731
        return lib.pbf_kzg_open_cells_each_bn254(h, q(xx), nn, ll, w(om), q(p), le, pitch, b, pbf._ptr(out_y), q(ww))

    for om in [F.root_of_unity(n), F.root_of_unity(4 * n), 0, 1, R, R + w2]:
        assert opn(om=om) == EINVAL and host(om=om) == EINVAL, om
    for nn in (0, 3, 6, 12, 1 << 28, 1 << 40):
        assert opn(nn=nn) == EINVAL and host(nn=nn) == EINVAL, nn
    for ll in (0, 3, 6, 2 * n, 1 << 40):
        assert opn(ll=ll) == EINVAL and host(ll=ll) == EINVAL, ll
    assert opn(le=0) == EINVAL and opn(le=n + 1, pitch=n + 1) == EINVAL
    assert host(le=0) == EINVAL and host(le=n + 1, pitch=n + 1) == EINVAL
    assert opn(pitch=ln - 1) == EINVAL and host(pitch=ln - 1) == EINVAL
    assert opn(b=0) == EINVAL and opn(b=(1 << 16) + 1) == EINVAL
    assert host(b=0) == EINVAL and host(b=(1 << 16) + 1) == EINVAL
    # batch * n = 2^24 + n, with the batch within its own limit
    big_n = 1 << 12
    assert opn(nn=big_n, om=omega2_of(big_n), b=(1 << 12) + 1) == EINVAL
    assert host(nn=big_n, om=omega2_of(big_n), b=(1 << 12) + 1) == EINVAL
    assert b"this version supports" in lib.pbf_last_error()
    assert opn(xx=None) == EINVAL and opn(om=None) == EINVAL and opn(p=None) == EINVAL
    assert opn(ww=None) == EINVAL and opn(ctxh=None) == EINVAL
    assert host(xx=None) == EINVAL and host(p=None) == EINVAL and host(ww=None) == EINVAL
    # nothing was enqueued or written
    world.torch.cuda.synchronize()
    assert not out_y.any() and not out_w.any()
    assert bool((d_y == -1).all()) and bool((d_w == -1).all())
    # and the same arguments, valid, succeed
    assert opn() == 0 and opn(y=None) == 0
    world.torch.cuda.synchronize()  # the host form runs on the context's own stream, over the same scratch
    assert host() == 0
    assert not bool((d_y == -1).all()) and not bool((d_w == -1).all())
    assert out_w.any() and np.array_equal(out_w.view(np.int64), d_w.cpu().numpy())
    assert np.array_equal(out_y.view(np.int64), d_y.cpu().numpy())
