"""Every opening at once (csrc/kzg_cells.hip pbf_kzg_fk20_setup_bn254*, pbf_kzg_open_all_bn254*),
bit-exact: no tolerance anywhere.

Expected values use the trapdoor S of the test SRS (tests/fk20_expect.py): xext = [NTT_2n(a)]G,
y_b[i] = p_b(omega^i), W_i = [(c(S) - c(omega^i)) / (S - omega^i)]G for c = sum_b w_b p_b, the
points through pbf_g1_bn254_mul_base_dev; and W_i, y must equal, word for word, what kzg_open
returns at z = omega^i.

Shapes. n = 1 and 2 are their own paths; n = 4 .. 256 walk 2n over the G1 NTT's boundaries (64
lanes per workgroup, position-major against group-major stages, the load's 256 threads: 2n = 64,
128, 256, 512); the window table's tile of 2^g1ntt.tile_log products is met by 2n = 2^15 at the
default (n = 2^13 below it, 2^14 at it) and by every size from 2n = 64 on with the option at 6
(n = 2^10: 32 launches for the pointwise product, 16 per stage)."""
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
import fk20_expect as K  # noqa: E402

pytestmark = pytest.mark.gpu
R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R  # the trapdoor
M = 1 << 14  # device SRS: M + 1 points
EINVAL = 1


def omega2_of(n):
    return F.root_of_unity(2 * n)


class World:
    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch
        self.d_srs = torch.empty(8 * (M + 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.srs_create_dev(S, M, self.d_srs.data_ptr())
        torch.cuda.synchronize()
        self._xext, self._host_srs = {}, None

    def host_srs(self, m):
        if self._host_srs is None:
            self._host_srs = self.points(self.d_srs[:8 * 65])
        return self._host_srs[:m]

    def scalars(self, ks):
        return self.torch.from_numpy(F.ints_to_limbs(ks).view(np.int64)).cuda()

    def mul_base(self, ks, ctx=None):
        d = self.scalars(ks)
        out = self.torch.empty(8 * len(ks), dtype=self.torch.int64, device="cuda")
        (ctx or self.ctx).g1_mul_base_dev(d.data_ptr(), out.data_ptr(), len(ks))
        self.torch.cuda.synchronize()
        return out

    def points(self, t):
        v = F.limbs_to_ints(t.cpu().numpy().view(np.uint64))
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def xext(self, ctx, n, omega2=None):
        """The setup of size n on the device, once per (context, n, omega2)."""
        omega2 = omega2 or omega2_of(n)
        key = (id(ctx), n, omega2)
        if key not in self._xext:
            out = self.torch.full((16 * n,), -1, dtype=self.torch.int64, device="cuda")
            self.torch.cuda.synchronize()
            ctx.kzg_fk20_setup_dev(self.d_srs.data_ptr(), M + 1, omega2, n, out.data_ptr())
            self.torch.cuda.synchronize()
            self._xext[key] = out
        return self._xext[key]

    def dev_polys(self, polys, pitch, seed=1):
        """The polynomials (lists of one length) at `pitch`, the gaps filled with random values."""
        a = F.random_limbs(len(polys) * pitch, seed)
        for b, p in enumerate(polys):
            a[4 * b * pitch:4 * (b * pitch + len(p))] = F.ints_to_limbs(p)
        return self.torch.from_numpy(a.view(np.int64)).cuda()

    def open_all(self, ctx, n, polys, weights, pitch=None, omega2=None, with_y=True, side_stream=False):
        """(y as lists or None, W as a tensor) of the device form."""
        torch = self.torch
        ln, batch = len(polys[0]), len(polys)
        pitch = pitch or ln
        d_p = self.dev_polys(polys, pitch)
        d_y = torch.full((4 * batch * n,), -1, dtype=torch.int64, device="cuda")
        d_w = torch.full((8 * n,), -1, dtype=torch.int64, device="cuda")
        x = self.xext(ctx, n, omega2)
        torch.cuda.synchronize()
        st = torch.cuda.Stream() if side_stream else None
        ctx.kzg_open_all_dev(x.data_ptr(), n, omega2 or omega2_of(n), d_p.data_ptr(), ln, pitch, batch, weights,
                             d_y.data_ptr() if with_y else 0, d_w.data_ptr(), stream=st.cuda_stream if st else 0)
        if st:
            st.synchronize()
        torch.cuda.synchronize()
        if not with_y:
            assert bool((d_y == -1).all())
            return None, d_w
        v = F.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
        return [v[b * n:(b + 1) * n] for b in range(batch)], d_w


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


@pytest.fixture(scope="module")
def tiled_ctx():
    import pbf

    c = pbf.Context(0, options={"g1ntt.tile_log": "6"})
    yield c
    c.close()


def expect(polys, weights, n):
    """([y_b], the scalars of W) in the trapdoor form."""
    omega = pow(omega2_of(n), 2, R)
    ys = [F.ntt(K.padded(p, n), omega) if n > 1 else [p[0] % R] for p in polys]
    c = K.combine(polys, weights, n)
    cs = F.poly_eval(c, S)
    cy = [sum(w * y[i] for w, y in zip(weights, ys)) % R for i in range(n)]  # c(omega^i), by linearity
    dens, w = [], 1
    for _ in range(n):
        dens.append((S - w) % R)
        w = w * omega % R
    return ys, [(cs - y) * d % R for y, d in zip(cy, K.inv_all(dens))]


def prover_weights(batch, n, rng):
    """1, z^(n+2), z^(2n+4), v, v^2, ... as the prover's opening has them, one of them zeroed."""
    z, v = rng.randrange(R), rng.randrange(R)
    w = [1, pow(z, n + 2, R), pow(z, 2 * n + 4, R)] + [pow(v, k, R) for k in range(1, batch)]
    w = w[:batch]
    if batch > 1:
        w[batch // 2] = 0
    return w


def random_polys(rng, batch, ln):
    return [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]


# ---------------------------------------------------------------- setup
@pytest.mark.parametrize("n", [1, 2, 4, 64])
def test_xext_is_the_transform_of_a(ctx, world, n):
    omega2 = omega2_of(n)
    srs = world.host_srs(max(n - 1, 0))
    a = [srs[n - 2 - t] if t <= n - 2 else (0, 0) for t in range(2 * n)]
    want = ctx.ntt_g1(omega2, a)
    assert ctx.kzg_fk20_setup(srs, n, omega2) == want
    assert world.points(world.xext(ctx, n)) == want
    assert want == world.points(world.mul_base(K.xext_scalars(n, S, omega2)))
    if n == 1:
        assert want == [(0, 0), (0, 0)]
    else:  # a longer SRS changes nothing: points past n - 2 are not read
        assert ctx.kzg_fk20_setup(world.host_srs(n + 1), n, omega2) == want


# ---------------------------------------------------------------- all openings
SIZES = [1, 2, 4, 8, 16, 32, 64, 128, 256, 1 << 13, 1 << 14]


def check_trapdoor(world, ctx, n, batch, ln, seed, pitch=None, side_stream=False):
    rng = random.Random(seed)
    polys = random_polys(rng, batch, ln)
    weights = prover_weights(batch, n, rng)
    ys, d_w = world.open_all(ctx, n, polys, weights, pitch=pitch, side_stream=side_stream)
    want_y, want_w = expect(polys, weights, n)
    assert ys == want_y
    assert world.torch.equal(d_w, world.mul_base(want_w))
    return polys, weights, ys, d_w


@pytest.mark.parametrize("n", SIZES)
def test_against_the_trapdoor_form(ctx, world, n):
    check_trapdoor(world, ctx, n, 1 if n > 256 else 1 + n % 3, n, 500 + n, side_stream=n in (8, 256))


def test_small_tiles(tiled_ctx, world):
    check_trapdoor(world, tiled_ctx, 1 << 10, 2, 1 << 10, 66)


@pytest.mark.parametrize("n", SIZES)
def test_against_kzg_open(ctx, world, n):
    """y and W against the single opening at z = omega^i: every i up to n = 64, four above."""
    rng = random.Random(900 + n)
    batch = 2 if n <= 256 else 1
    polys = random_polys(rng, batch, n)
    weights = prover_weights(batch, n, rng)
    ys, d_w = world.open_all(ctx, n, polys, weights)
    got_w = world.points(d_w)
    omega = pow(omega2_of(n), 2, R)
    d_p = world.dev_polys(polys, n)
    for i in (range(n) if n <= 64 else (0, 1, n // 2, n - 1)):
        z = pow(omega, i, R)
        if n <= 64:  # the host form below, the device form above
            y1, w1 = ctx.kzg_open(world.host_srs(n), polys, z, weights)
        else:
            y1, w1 = ctx.kzg_open_dev(world.d_srs.data_ptr(), M + 1, d_p.data_ptr(), n, n, batch, z, weights)
        assert [y[i] for y in ys] == y1, (n, i)
        assert got_w[i] == w1, (n, i)


@pytest.mark.parametrize("n", [16, 64])
def test_lengths(ctx, world, n):
    for ln in (1, 2, n // 2 + 1, n - 1, n):
        polys, _, ys, d_w = check_trapdoor(world, ctx, n, 2, ln, 40 * n + ln)
        if ln == 1:
            assert not bool(d_w.any())  # every W the identity
            assert ys == [[p[0]] * n for p in polys]  # y constant


@pytest.mark.parametrize("n", [1, 2, 64])
def test_zero_polynomial(ctx, world, n):
    for ln in {1, n}:
        ys, d_w = world.open_all(ctx, n, [[0] * ln], [7])
        assert ys == [[0] * n] and not bool(d_w.any())
    # and zero weights on a polynomial that is not
    _, d_w = world.open_all(ctx, n, [[5] * n, [9] * n], [0, 0])
    assert not bool(d_w.any())


@pytest.mark.parametrize("batch", [1, 6, 11])
def test_batches_and_pitch(ctx, world, batch):
    """Batch 1 and 6 with the prover's weights, 11 for the second launch of the linear
    combination; compact and with pitch > len."""
    n, ln = 32, 29
    a = check_trapdoor(world, ctx, n, batch, ln, 7 + batch)
    b = check_trapdoor(world, ctx, n, batch, ln, 7 + batch, pitch=ln + 5)
    assert world.torch.equal(a[3], b[3])


def test_host_form(ctx, world):
    n, rng = 16, random.Random(12)
    polys = random_polys(rng, 3, n - 2)
    weights = prover_weights(3, n, rng)
    xext = world.points(world.xext(ctx, n))
    want_y, want_w = expect(polys, weights, n)
    want_pts = world.points(world.mul_base(want_w))
    assert ctx.kzg_open_all(xext, omega2_of(n), polys, weights) == (want_y, want_pts)
    assert ctx.kzg_open_all(xext, omega2_of(n), polys, weights, pitch=n + 1) == (want_y, want_pts)
    assert ctx.kzg_open_all(xext, omega2_of(n), polys, weights, with_y=False) == (None, want_pts)
    assert ctx.kzg_open_all([(0, 0), (0, 0)], R - 1, [[5], [6]], [1, 1]) == ([[5], [6]], [(0, 0)])


def test_verifies(ctx, world):
    n, rng = 8, random.Random(3)
    polys = random_polys(rng, 1, n)
    ys, d_w = world.open_all(ctx, n, polys, [1])
    ws = world.points(d_w)
    g2s = [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [S])[0]]
    d_p = world.dev_polys(polys, n)
    commit = ctx.kzg_commit_dev(world.d_srs.data_ptr(), M + 1, d_p.data_ptr(), n, n, 1)[0]
    omega = pow(omega2_of(n), 2, R)
    entries = [(commit, pow(omega, i, R), ys[0][i], ws[i]) for i in (0, 3, 7)]
    rhos = [1] + [rng.randrange(1, R) for _ in entries[1:]]
    assert ctx.kzg_verify(g2s, entries, rhos)
    bad = list(entries)
    bad[1] = (commit, entries[1][1], (entries[1][2] + 1) % R, entries[1][3])
    assert not ctx.kzg_verify(g2s, bad, rhos)
    assert not ctx.kzg_verify(g2s, [bad[1]], [1])


@pytest.mark.parametrize("n", [2, 16])
def test_both_roots_of_omega(ctx, world, n):
    rng = random.Random(n)
    polys = random_polys(rng, 2, n)
    w2 = omega2_of(n)
    ya, wa = world.open_all(ctx, n, polys, [3, 4])
    yb, wb = world.open_all(ctx, n, polys, [3, 4], omega2=R - w2)
    assert ya == yb and world.torch.equal(wa, wb)
    if n > 2:  # at n = 2 a is the single point G, and its transform the same for every root
        assert not world.torch.equal(world.xext(ctx, n), world.xext(ctx, n, R - w2))


def test_without_y(ctx, world):
    n, rng = 64, random.Random(64)
    polys = random_polys(rng, 2, n)
    _, with_y = world.open_all(ctx, n, polys, [1, 2])
    none, without = world.open_all(ctx, n, polys, [1, 2], with_y=False)
    assert none is None and world.torch.equal(with_y, without)


def test_errors(ctx, world):
    import pbf

    lib, h = ctx.lib, ctx.h
    n, ln, batch = 8, 8, 2
    vp = ctypes.c_void_p
    w = lambda v: pbf._ptr(pbf.ints_to_limbs(v if isinstance(v, list) else [v]))  # noqa: E731
    w2 = omega2_of(n)
    x = world.xext(ctx, n)
    d_p = world.dev_polys(random_polys(random.Random(1), batch, ln), ln)
    d_y = world.torch.full((4 * batch * n,), -1, dtype=world.torch.int64, device="cuda")
    d_w = world.torch.full((8 * n,), -1, dtype=world.torch.int64, device="cuda")
    d_x = world.torch.full((16 * n,), -1, dtype=world.torch.int64, device="cuda")
    world.torch.cuda.synchronize()
    srs = vp(world.d_srs.data_ptr())

    def setup(s=srs, m=M + 1, om=w2, nn=n, out=vp(d_x.data_ptr()), ctxh=h):
        return lib.pbf_kzg_fk20_setup_bn254_dev(ctxh, s, m, w(om) if om is not None else None, nn, out, None)

    def opn(xx=vp(x.data_ptr()), nn=n, om=w2, p=vp(d_p.data_ptr()), l=ln, pitch=ln, b=batch, wt=[1, 2],
            y=vp(d_y.data_ptr()), ww=vp(d_w.data_ptr()), ctxh=h):
        return lib.pbf_kzg_open_all_bn254_dev(ctxh, xx, nn, w(om) if om is not None else None, p, l, pitch, b,
                                              w(wt) if wt is not None else None, y, ww, None)

    bad_roots = [F.root_of_unity(n), F.root_of_unity(4 * n), 0, 1, R, R + w2]
    for om in bad_roots:
        assert setup(om=om) == EINVAL, om
        assert opn(om=om) == EINVAL, om
    for nn in (0, 3, 6, 12, 1 << 28, 1 << 40):
        assert setup(nn=nn) == EINVAL, nn
        assert opn(nn=nn) == EINVAL, nn
    assert setup(nn=1 << 28, om=F.root_of_unity(1 << 28)) == EINVAL  # 2n is past the 2-adicity
    assert setup(m=n - 2) == EINVAL  # needs n - 1 points
    assert setup(s=None) == EINVAL and setup(om=None) == EINVAL and setup(out=None) == EINVAL
    assert setup(ctxh=None) == EINVAL
    assert opn(l=0) == EINVAL and opn(l=n + 1, pitch=n + 1) == EINVAL
    assert opn(pitch=ln - 1) == EINVAL
    assert opn(b=0) == EINVAL and opn(b=(1 << 16) + 1) == EINVAL
    assert opn(wt=[1, R]) == EINVAL
    assert opn(xx=None) == EINVAL and opn(om=None) == EINVAL and opn(p=None) == EINVAL
    assert opn(wt=None) == EINVAL and opn(ww=None) == EINVAL and opn(ctxh=None) == EINVAL
    # the host forms: a setup point off the curve
    hs = world.host_srs(n - 1)
    off = list(hs)
    off[3] = (hs[3][0], (hs[3][1] + 1) % F.Q)
    out = np.zeros(16 * n, dtype=np.uint64)
    assert lib.pbf_kzg_fk20_setup_bn254(h, pbf._ptr(pbf._g1_limbs(off)), n - 1, w(w2), n, pbf._ptr(out)) == EINVAL
    assert lib.pbf_kzg_fk20_setup_bn254(h, pbf._ptr(pbf._g1_limbs(hs)), n - 2, w(w2), n, pbf._ptr(out)) == EINVAL
    # nothing was enqueued or written
    world.torch.cuda.synchronize()
    assert not out.any()
    assert bool((d_y == -1).all()) and bool((d_w == -1).all()) and bool((d_x == -1).all())
    # and the same arguments, valid, succeed; the minimal SRS is enough
    assert setup(m=n - 1) == 0 and opn() == 0 and opn(y=None) == 0
    world.torch.cuda.synchronize()
    assert world.torch.equal(d_x, x)
    assert ctx.kzg_fk20_setup(hs, n, w2) == world.points(x)
