"""KZG cell proofs (csrc/kzg_cells.hip pbf_kzg_cells_setup_bn254*, pbf_kzg_open_cells_bn254*,
pbf_kzg_verify_cells_bn254), bit-exact: no tolerance anywhere.

Expected values use the trapdoor S of the test SRS (tests/fk20_cells_expect.py): xext =
[NTT_2k(a_r)]G slab after slab, ys[b][i][t] = p_b(omega^(i + k t)), W_i = [q_i(S)]G for the quotient
of c = sum_b w_b p_b by x^l - c_i from long division, the points through
pbf_g1_bn254_mul_base_dev.

Shapes. Every (n, l) with l <= n <= 64 checks every cell: l = 1 is FK20 itself and l = n the
identities. 2k = 64 .. 512 at l = 2 walk the G1 NTT's boundaries (64 lanes per workgroup,
position-major against group-major stages, the load's 256 threads); at l = 64, n = 2^11 .. 2^14 do
the same with 64-term sums, the last meeting the window table's default tile with 2n = 2^15. With
g1ntt.tile_log = 6 at n = 2^10 the slabs of one frequency lie in different launches of the product.
Above n = 64 a sample of 16 cells is checked (the Python expectations are O(n) per cell)."""
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
M = 1 << 14  # device SRS: M + 1 points
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
        self._xext, self._host_srs, self._g2 = {}, None, {}

    def host_srs(self, m):
        if self._host_srs is None:
            self._host_srs = self.points(self.d_srs[:8 * 65])
        return self._host_srs[:m]

    def g2s(self, l):
        """[G2, [s^l]G2], the l-th power from the trapdoor."""
        if l not in self._g2:
            self._g2[l] = [B.G2_GEN, self.ctx.g2_bn254_mul([B.G2_GEN], [pow(S, l, R)])[0]]
        return self._g2[l]

    def scalars(self, ks):
        return self.torch.from_numpy(F.ints_to_limbs(ks).view(np.int64)).cuda()

    def mul_base(self, ks):
        d = self.scalars(ks)
        out = self.torch.empty(8 * len(ks), dtype=self.torch.int64, device="cuda")
        self.ctx.g1_mul_base_dev(d.data_ptr(), out.data_ptr(), len(ks))
        self.torch.cuda.synchronize()
        return out

    def points(self, t):
        v = F.limbs_to_ints(t.cpu().numpy().view(np.uint64))
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def xext(self, ctx, n, l, omega2=None):
        """The setup of (n, l) on the device, once per (context, n, l, omega2)."""
        omega2 = omega2 or omega2_of(n)
        key = (id(ctx), n, l, omega2)
        if key not in self._xext:
            out = self.torch.full((16 * n,), -1, dtype=self.torch.int64, device="cuda")
            self.torch.cuda.synchronize()
            ctx.kzg_cells_setup_dev(self.d_srs.data_ptr(), M + 1, omega2, n, l, out.data_ptr())
            self.torch.cuda.synchronize()
            self._xext[key] = out
        return self._xext[key]

    def dev_polys(self, polys, pitch, seed=1):
        """The polynomials (lists of one length) at `pitch`, the gaps filled with random values."""
        a = F.random_limbs(len(polys) * pitch, seed)
        for b, p in enumerate(polys):
            a[4 * b * pitch:4 * (b * pitch + len(p))] = F.ints_to_limbs(p)
        return self.torch.from_numpy(a.view(np.int64)).cuda()

    def open_cells(self, ctx, n, l, polys, weights, pitch=None, omega2=None, with_y=True, side_stream=False):
        """(ys[b][i] as lists of l values or None, W as a tensor of k points) of the device form."""
        torch = self.torch
        ln, batch, k = len(polys[0]), len(polys), n // l
        pitch = pitch or ln
        d_p = self.dev_polys(polys, pitch)
        d_y = torch.full((4 * batch * n,), -1, dtype=torch.int64, device="cuda")
        d_w = torch.full((8 * k,), -1, dtype=torch.int64, device="cuda")
        x = self.xext(ctx, n, l, omega2)
        torch.cuda.synchronize()
        st = torch.cuda.Stream() if side_stream else None
        ctx.kzg_open_cells_dev(x.data_ptr(), n, l, omega2 or omega2_of(n), d_p.data_ptr(), ln, pitch, batch, weights,
                               d_y.data_ptr() if with_y else 0, d_w.data_ptr(), stream=st.cuda_stream if st else 0)
        if st:
            st.synchronize()
        torch.cuda.synchronize()
        if not with_y:
            assert bool((d_y == -1).all())
            return None, d_w
        v = F.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
        return [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)], d_w

    def commit(self, p):
        d_p = self.dev_polys([p], len(p))
        return self.ctx.kzg_commit_dev(self.d_srs.data_ptr(), M + 1, d_p.data_ptr(), len(p), len(p), 1)[0]


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


@pytest.fixture(scope="module")
def tiled_ctx():
    import pbf

    c = pbf.Context(0, options={"g1ntt.tile_log": "6"})
    yield c
    c.close()


def sample_cells(k):
    """Every cell up to 64 of them, else 16 with the first and the last."""
    if k <= 64:
        return list(range(k))
    return sorted({0, 1, k // 2 - 1, k // 2, k - 2, k - 1} | set(random.Random(k).sample(range(k), 10)))


def expect_w(polys, weights, n, l, cells):
    """The scalars of W_i for i in cells, by long division of c = sum_b w_b p_b by x^l - c_i."""
    omega, c = omega_of(n), K.combine(polys, weights, n)
    return [F.poly_eval(C.divide(c, l, pow(omega, i * l, R))[0] or [0], S) for i in cells]


def random_polys(rng, batch, ln):
    return [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]


def prover_weights(batch, n, rng):
    """1, z^(n+2), z^(2n+4), v, v^2, ... as the prover's opening has them, one of them zeroed."""
    z, v = rng.randrange(R), rng.randrange(R)
    w = [1, pow(z, n + 2, R), pow(z, 2 * n + 4, R)] + [pow(v, k, R) for k in range(1, batch)]
    w = w[:batch]
    if batch > 1:
        w[batch // 2] = 0
    return w


def check(world, ctx, n, l, polys, weights, **kw):
    """One call against the expectations: every value, and W on the sampled cells."""
    k = n // l
    cells = sample_cells(k)
    ys, d_w = world.open_cells(ctx, n, l, polys, weights, **kw)
    if ys is not None:
        assert ys == [C.cell_values(p, n, l, omega_of(n)) for p in polys]
    want = world.mul_base(expect_w(polys, weights, n, l, cells))
    assert world.torch.equal(d_w.view(k, 8)[cells], want.view(len(cells), 8)), (n, l)
    return ys, d_w


def check_random(world, ctx, n, l, batch, ln, seed, **kw):
    rng = random.Random(seed)
    polys = random_polys(rng, batch, ln)
    weights = prover_weights(batch, n, rng)
    return (polys, weights) + check(world, ctx, n, l, polys, weights, **kw)


# ---------------------------------------------------------------- every shape up to n = 64
POW2 = [1, 2, 4, 8, 16, 32, 64]
SHAPES = [(n, l) for n in POW2 for l in POW2 if l <= n]


@pytest.mark.parametrize("n,l", SHAPES)
def test_every_shape(ctx, world, n, l):
    k, omega2 = n // l, omega2_of(n)
    # xext: the G1 NTT of each a_r, and the trapdoor's scalars
    x = world.xext(ctx, n, l)
    got_x = world.points(x)
    srs = world.host_srs(n - l)
    w = pow(omega2, l, R)
    for r in range(l):
        a = [srs[r + l * (k - 2 - t)] if t <= k - 2 else (0, 0) for t in range(2 * k)]
        assert got_x[r * 2 * k:(r + 1) * 2 * k] == ctx.ntt_g1(w, a), (n, l, r)
    assert world.torch.equal(x, world.mul_base(C.xext_scalars(n, l, S, omega2)))
    assert ctx.kzg_cells_setup(srs, n, l, omega2) == got_x  # the host form, on the minimal SRS
    polys, weights, ys, d_w = check_random(world, ctx, n, l, 2, n, 100 * n + l, side_stream=(n, l) in ((64, 8), (8, 2)))
    if l == n:  # one cell: the whole domain; the quotient is zero
        assert not bool(x.any()) and not bool(d_w.any())
    if l == 1:  # FK20 itself, word for word
        torch = world.torch
        x20 = torch.full((16 * n,), -1, dtype=torch.int64, device="cuda")
        d_y = torch.full((8 * n,), -1, dtype=torch.int64, device="cuda")
        d_w20 = torch.full((8 * n,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.kzg_fk20_setup_dev(world.d_srs.data_ptr(), M + 1, omega2, n, x20.data_ptr())
        d_p = world.dev_polys(polys, n)
        ctx.kzg_open_all_dev(x20.data_ptr(), n, omega2, d_p.data_ptr(), n, n, 2, weights, d_y.data_ptr(), d_w20.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(x, x20) and torch.equal(d_w, d_w20)
        v = F.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
        assert [[c[0] for c in y] for y in ys] == [v[:n], v[n:]]


# ---------------------------------------------------------------- transform boundaries
@pytest.mark.parametrize("n,l", [(64, 2), (128, 2), (256, 2), (512, 2), (1 << 11, 64), (1 << 12, 64), (1 << 13, 64),
                                 (1 << 14, 64)])
def test_transform_boundaries(ctx, world, n, l):
    check_random(world, ctx, n, l, 1, n, 7 * n + l)


@pytest.mark.parametrize("l", [4, 64])
def test_small_tiles(tiled_ctx, world, l):
    """tile_log = 6 at n = 2^10: 32 launches for the 2n products, the l slabs of one frequency in
    different ones."""
    check_random(world, tiled_ctx, 1 << 10, l, 2, 1 << 10, 66 + l)


# ---------------------------------------------------------------- the exits of the sum
@pytest.mark.parametrize("l", [2, 8])
def test_sum_of_equal_products(ctx, world, l):
    """p_(2u) = S p_(2u+1): slabs r and r + 1 (r even) have equal products at every frequency, so
    the sum meets P + P."""
    n, rng = 64, random.Random(l)
    odd = [rng.randrange(1, R) for _ in range(n // 2)]
    p = [v for o in odd for v in (S * o % R, o)]
    _, d_w = check(world, ctx, n, l, [p], [1])
    assert bool(d_w.any())


@pytest.mark.parametrize("l", [2, 8])
def test_sum_of_opposite_products(ctx, world, l):
    """p_(2u) = -S p_(2u+1): the products of slabs r and r + 1 cancel at every frequency (P + (-P),
    then the identity as an operand), and every W is the identity."""
    n, rng = 64, random.Random(10 + l)
    odd = [rng.randrange(1, R) for _ in range(n // 2)]
    p = [v for o in odd for v in ((R - S) * o % R, o)]
    _, d_w = check(world, ctx, n, l, [p], [1])
    assert not bool(d_w.any())


@pytest.mark.parametrize("l", [2, 8])
def test_one_residue_class(ctx, world, l):
    """A polynomial supported on one residue class mod l: every other slab contributes the
    identity, first, in the middle or last in the sum."""
    n, rng = 64, random.Random(20 + l)
    for r in (0, l // 2, l - 1):
        p = [rng.randrange(1, R) if j % l == r else 0 for j in range(n)]
        _, d_w = check(world, ctx, n, l, [p], [1])
        assert bool(d_w.any())


# ---------------------------------------------------------------- lengths, batches, call forms
def test_lengths(ctx, world):
    n, l = 64, 8
    for ln in (1, l, l + 1, n - 1, n):
        polys, _, ys, d_w = check_random(world, ctx, n, l, 2, ln, 40 * n + ln)
        assert bool(d_w.any()) == (ln > l)  # degree below l: every quotient is zero
        if ln == 1:
            assert ys == [[[p[0]] * l] * (n // l) for p in polys]


@pytest.mark.parametrize("n,l", [(1, 1), (8, 8), (64, 8)])
def test_zero_polynomial(ctx, world, n, l):
    for ln in {1, n}:
        ys, d_w = world.open_cells(ctx, n, l, [[0] * ln], [7])
        assert ys == [[[0] * l] * (n // l)] and not bool(d_w.any())
    # and zero weights on a polynomial that is not
    _, d_w = world.open_cells(ctx, n, l, [[5] * n, [9] * n], [0, 0])
    assert not bool(d_w.any())


@pytest.mark.parametrize("batch", [1, 6, 11])
def test_batches_and_pitch(ctx, world, batch):
    """Batch 1 and 6 with the prover's weights, 11 for the second launch of the linear
    combination; compact and with pitch > len; and the batch against one call on the combined
    polynomial."""
    n, l, ln = 64, 8, 61
    polys, weights, _, d_w = check_random(world, ctx, n, l, batch, ln, 7 + batch)
    b = check_random(world, ctx, n, l, batch, ln, 7 + batch, pitch=ln + 5)
    assert world.torch.equal(d_w, b[3])
    _, single = world.open_cells(ctx, n, l, [K.combine(polys, weights, n)], [1])
    assert world.torch.equal(d_w, single)


def test_without_y(ctx, world):
    n, l, rng = 64, 8, random.Random(64)
    polys = random_polys(rng, 2, n)
    _, with_y = world.open_cells(ctx, n, l, polys, [1, 2])
    none, without = world.open_cells(ctx, n, l, polys, [1, 2], with_y=False)
    assert none is None and world.torch.equal(with_y, without)


@pytest.mark.parametrize("n,l", [(16, 1), (16, 4), (64, 8)])
def test_both_roots_of_omega(ctx, world, n, l):
    rng = random.Random(n + l)
    polys = random_polys(rng, 2, n)
    w2 = omega2_of(n)
    ya, wa = world.open_cells(ctx, n, l, polys, [3, 4])
    yb, wb = world.open_cells(ctx, n, l, polys, [3, 4], omega2=R - w2)
    assert ya == yb and world.torch.equal(wa, wb)
    if l == 1:  # with l even both roots have the same l-th power, and the same xext
        assert not world.torch.equal(world.xext(ctx, n, l), world.xext(ctx, n, l, R - w2))
    else:
        assert world.torch.equal(world.xext(ctx, n, l), world.xext(ctx, n, l, R - w2))


def test_host_form(ctx, world):
    n, l, rng = 32, 4, random.Random(12)
    k = n // l
    polys = random_polys(rng, 3, n - 2)
    weights = prover_weights(3, n, rng)
    xext = world.points(world.xext(ctx, n, l))
    want_y = [C.cell_values(p, n, l, omega_of(n)) for p in polys]
    want_w = world.points(world.mul_base(expect_w(polys, weights, n, l, range(k))))
    assert ctx.kzg_open_cells(xext, l, omega2_of(n), polys, weights) == (want_y, want_w)
    assert ctx.kzg_open_cells(xext, l, omega2_of(n), polys, weights, pitch=n + 1) == (want_y, want_w)
    assert ctx.kzg_open_cells(xext, l, omega2_of(n), polys, weights, with_y=False) == (None, want_w)
    assert ctx.kzg_open_cells([(0, 0), (0, 0)], 1, R - 1, [[5], [6]], [1, 1]) == ([[[5]], [[6]]], [(0, 0)])
    # a longer SRS changes nothing: points past n - l - 1 are not read
    assert ctx.kzg_cells_setup(world.host_srs(n + 1), n, l, omega2_of(n)) == xext


# ---------------------------------------------------------------- verification
class Proven:
    """Two polynomials of size n opened in cells of l, with their commitments."""

    def __init__(self, world, ctx, n, l, seed):
        rng = random.Random(seed)
        self.n, self.l, self.k, self.omega = n, l, n // l, omega_of(n)
        self.polys = random_polys(rng, 2, n)
        self.commits = [world.commit(p) for p in self.polys]
        self.ys, self.ws = [], []
        for p in self.polys:
            y, d_w = world.open_cells(ctx, n, l, [p], [1])
            self.ys.append(y[0])
            self.ws.append(world.points(d_w))
        self.g2s, self.srs, self.rng = world.g2s(l), world.host_srs(l), rng

    def entry(self, b, i):
        return (self.commits[b], i, self.ys[b][i], self.ws[b][i])

    def rhos(self, count):
        return [self.rng.randrange(1, R) for _ in range(count)]

    def verify(self, ctx, entries, rhos=None, g2s=None):
        return ctx.kzg_verify_cells(g2s or self.g2s, self.srs, self.omega, self.n, self.l, entries,
                                    rhos or self.rhos(len(entries)))


@pytest.fixture(scope="module", params=[(64, 8), (1024, 64)], ids=["64x8", "1024x64"])
def proven(request, ctx, world):
    n, l = request.param
    return Proven(world, ctx, n, l, n + l)


def test_verify_accepts(ctx, proven):
    k = proven.k
    every = [proven.entry(0, i) for i in range(k)]
    assert proven.verify(ctx, every)
    assert proven.verify(ctx, every[1::3])  # a subset
    assert proven.verify(ctx, [every[k - 1]], [1])  # one cell
    assert proven.verify(ctx, [every[2], every[5], every[2]])  # a repeated cell
    assert proven.verify(ctx, [proven.entry(0, 1), proven.entry(1, 1), proven.entry(1, k - 1), proven.entry(0, 0)])


def test_verify_rejects(ctx, world, proven):
    k, l = proven.k, proven.l
    good = [proven.entry(0, 0), proven.entry(1, 3), proven.entry(0, k - 1)]
    rhos = proven.rhos(3)
    assert proven.verify(ctx, good, rhos)
    c, i, ys, w = good[1]
    for t in (0, l - 1):  # one changed value
        bad_ys = list(ys)
        bad_ys[t] = (bad_ys[t] + 1) % R
        assert not proven.verify(ctx, [good[0], (c, i, bad_ys, w), good[2]], rhos)
    assert not proven.verify(ctx, [good[0], (c, i, ys, proven.ws[1][4]), good[2]], rhos)  # a changed W
    assert not proven.verify(ctx, [good[0], (proven.commits[0], i, ys, w), good[2]], rhos)  # a changed C
    assert not proven.verify(ctx, [good[0], (c, i + 1, ys, w), good[2]], rhos)  # a wrong cell_idx
    assert not proven.verify(ctx, [(c, i, bad_ys, w)], [1])  # a bad entry on its own
    assert not proven.verify(ctx, good, rhos, g2s=world.g2s(1))  # [s]G2 in place of [s^l]G2
    off = (w[0], (w[1] + 1) % F.Q)  # a point off the curve
    assert not proven.verify(ctx, [good[0], (c, i, ys, off), good[2]], rhos)
    assert not proven.verify(ctx, [good[0], (off, i, ys, w), good[2]], rhos)
    assert not proven.verify(ctx, [good[0], ((F.Q, 2), i, ys, w), good[2]], rhos)  # not canonical
    srs = list(proven.srs)
    srs[l - 1] = off
    assert not ctx.kzg_verify_cells(proven.g2s, srs, proven.omega, proven.n, l, good, rhos)


def cyclic_entries(proven, count):
    """count entries: the cells of both polynomials, repeated cyclically"""
    return [proven.entry(j % 2, (j // 2) % proven.k) for j in range(count)]


def with_changed_value(entry, t=0):
    c, i, ys, w = entry
    bad_ys = list(ys)
    bad_ys[t] = (bad_ys[t] + 1) % R
    return (c, i, bad_ys, w)


only_64x8 = pytest.mark.parametrize("proven", [(64, 8)], indirect=True, ids=["64x8"])


@only_64x8
@pytest.mark.parametrize("count", [32, 33, 257])
def test_verify_accepts_many_entries(ctx, proven, count):
    """32 entries fill one chunk of k_cells_vsweep (CV_CH), 33 leave one entry alone in a second
    chunk, so that k_cells_vsum adds two; 257 are two workgroups of k_cells_vprep, one live lane in
    the second, and nine chunks."""
    assert proven.verify(ctx, cyclic_entries(proven, count))


@only_64x8
@pytest.mark.parametrize("count,pos", [(33, 32), (257, 256)])
def test_verify_rejects_a_changed_value_in_the_last_entry(ctx, proven, count, pos):
    good, rhos = cyclic_entries(proven, count), proven.rhos(count)
    bad = list(good)
    bad[pos] = with_changed_value(good[pos], proven.l - 1)
    assert not proven.verify(ctx, bad, rhos)
    assert proven.verify(ctx, good, rhos)


@only_64x8
def test_verify_rejects_an_off_curve_w_in_the_second_workgroup(ctx, proven):
    good, rhos = cyclic_entries(proven, 257), proven.rhos(257)
    c, i, ys, w = good[256]
    off = (w[0], (w[1] + 1) % F.Q)
    assert not F.g1_on_curve(off)
    assert not proven.verify(ctx, good[:256] + [(c, i, ys, off)], rhos)


def test_equal_rho_lets_errors_cancel(ctx, proven):
    """DOCUMENTED, not a defect: the library reads no randomness. The same cell twice, one value
    raised by d in one copy and lowered by d in the other, passes under rho = 1, 1 and fails under
    weights chosen after the fact (include/pbf.h, the randomness contract)."""
    c, i, ys, w = proven.entry(0, 2)
    up, down = list(ys), list(ys)
    up[1], down[1] = (ys[1] + 5) % R, (ys[1] - 5) % R
    pair = [(c, i, up, w), (c, i, down, w)]
    assert proven.verify(ctx, pair, [1, 1])
    assert not proven.verify(ctx, pair, [1, 2])


def test_cells_of_one_are_point_openings(ctx, world):
    """With l = 1 a cell is a point: the verdicts agree with pbf_kzg_verify_bn254 on the same entries."""
    n = 16
    pv = Proven(world, ctx, n, 1, 5)
    cells = [pv.entry(0, 3), pv.entry(1, 0), pv.entry(0, 15)]
    rhos = pv.rhos(3)
    c, i, ys, w = cells[1]
    for entries in (cells, [cells[0], (c, i, [(ys[0] + 1) % R], w), cells[2]], [cells[0], (c, i + 1, ys, w), cells[2]]):
        points = [(e[0], pow(pv.omega, e[1], R), e[2][0], e[3]) for e in entries]
        assert pv.verify(ctx, entries, rhos) == ctx.kzg_verify(pv.g2s, points, rhos) == (entries is cells)


# ---------------------------------------------------------------- errors
def test_prover_errors(ctx, world):
    import pbf

    lib, h = ctx.lib, ctx.h
    n, l, ln, batch = 16, 4, 16, 2
    vp = ctypes.c_void_p
    w = lambda v: pbf._ptr(pbf.ints_to_limbs(v if isinstance(v, list) else [v]))  # noqa: E731
    w2 = omega2_of(n)
    x = world.xext(ctx, n, l)
    d_p = world.dev_polys(random_polys(random.Random(1), batch, ln), ln)
    d_y = world.torch.full((4 * batch * n,), -1, dtype=world.torch.int64, device="cuda")
    d_w = world.torch.full((8 * (n // l),), -1, dtype=world.torch.int64, device="cuda")
    d_x = world.torch.full((16 * n,), -1, dtype=world.torch.int64, device="cuda")
    world.torch.cuda.synchronize()
    srs = vp(world.d_srs.data_ptr())

    def setup(s=srs, m=M + 1, om=w2, nn=n, ll=l, out=vp(d_x.data_ptr()), ctxh=h):
        return lib.pbf_kzg_cells_setup_bn254_dev(ctxh, s, m, w(om) if om is not None else None, nn, ll, out, None)

    def opn(xx=vp(x.data_ptr()), nn=n, ll=l, om=w2, p=vp(d_p.data_ptr()), le=ln, pitch=ln, b=batch, wt=[1, 2],
            y=vp(d_y.data_ptr()), ww=vp(d_w.data_ptr()), ctxh=h):
        return lib.pbf_kzg_open_cells_bn254_dev(ctxh, xx, nn, ll, w(om) if om is not None else None, p, le, pitch, b,
                                                w(wt) if wt is not None else None, y, ww, None)

    for om in [F.root_of_unity(n), F.root_of_unity(4 * n), 0, 1, R, R + w2]:
        assert setup(om=om) == EINVAL, om
        assert opn(om=om) == EINVAL, om
    for nn in (0, 3, 6, 12, 1 << 28, 1 << 40):
        assert setup(nn=nn) == EINVAL, nn
        assert opn(nn=nn) == EINVAL, nn
    for ll in (0, 3, 6, 2 * n, 1 << 40):
        assert setup(ll=ll) == EINVAL, ll
        assert opn(ll=ll) == EINVAL, ll
    assert setup(m=n - l - 1) == EINVAL  # needs n - l points
    assert setup(s=None) == EINVAL and setup(om=None) == EINVAL and setup(out=None) == EINVAL
    assert setup(ctxh=None) == EINVAL
    assert opn(le=0) == EINVAL and opn(le=n + 1, pitch=n + 1) == EINVAL
    assert opn(pitch=ln - 1) == EINVAL
    assert opn(b=0) == EINVAL and opn(b=(1 << 16) + 1) == EINVAL
    assert opn(wt=[1, R]) == EINVAL
    assert opn(xx=None) == EINVAL and opn(om=None) == EINVAL and opn(p=None) == EINVAL
    assert opn(wt=None) == EINVAL and opn(ww=None) == EINVAL and opn(ctxh=None) == EINVAL
    # the host forms: a setup point off the curve, a short SRS
    hs = world.host_srs(n - l)
    off = list(hs)
    off[3] = (hs[3][0], (hs[3][1] + 1) % F.Q)
    out = np.zeros(16 * n, dtype=np.uint64)
    assert lib.pbf_kzg_cells_setup_bn254(h, pbf._ptr(pbf._g1_limbs(off)), n - l, w(w2), n, l, pbf._ptr(out)) == EINVAL
    assert lib.pbf_kzg_cells_setup_bn254(h, pbf._ptr(pbf._g1_limbs(hs)), n - l - 1, w(w2), n, l, pbf._ptr(out)) == EINVAL
    # nothing was enqueued or written
    world.torch.cuda.synchronize()
    assert not out.any()
    assert bool((d_y == -1).all()) and bool((d_w == -1).all()) and bool((d_x == -1).all())
    # and the same arguments, valid, succeed; the minimal SRS is enough
    assert setup(m=n - l) == 0 and opn() == 0 and opn(y=None) == 0
    world.torch.cuda.synchronize()
    assert world.torch.equal(d_x, x)


def test_verifier_errors(ctx, world):
    import pbf

    lib, h = ctx.lib, ctx.h
    n, l = 16, 4
    pv = Proven(world, ctx, n, l, 9)
    entries = [pv.entry(0, 1), pv.entry(1, 3)]
    limbs, g1 = pbf.ints_to_limbs, pbf._g1_limbs
    base = dict(ctxh=h, g2=pbf._g2_limbs(pv.g2s), srs=g1(pv.srs), m=l, om=limbs([pv.omega]), nn=n, ll=l, count=2,
                commits=g1([e[0] for e in entries]), idx=np.array([e[1] for e in entries], dtype=np.uint64),
                ys=limbs([v for e in entries for v in e[2]]), w=g1([e[3] for e in entries]), rho=limbs([3, 4]))

    def ver(**kw):
        a = dict(base, **kw)
        ok = ctypes.c_int(-1)
        p = lambda v: None if v is None else pbf._ptr(v)  # noqa: E731
        rc = lib.pbf_kzg_verify_cells_bn254(a["ctxh"], p(a["g2"]), p(a["srs"]), a["m"], p(a["om"]), a["nn"], a["ll"],
                                            a["count"], p(a["commits"]), p(a["idx"]), p(a["ys"]), p(a["w"]),
                                            p(a["rho"]), ctypes.byref(ok))
        return rc, ok.value

    assert ver() == (0, 1)
    for name in ("g2", "srs", "om", "commits", "idx", "ys", "w", "rho"):
        assert ver(**{name: None})[0] == EINVAL, name
    assert ver(ctxh=None)[0] == EINVAL
    for ll in (0, 3, 2 * n):
        assert ver(ll=ll)[0] == EINVAL, ll
    for nn in (0, 12, 1 << 28):
        assert ver(nn=nn)[0] == EINVAL, nn
    for om in (F.root_of_unity(2 * n), F.root_of_unity(n // 2), 0, 1, R):
        assert ver(om=limbs([om]))[0] == EINVAL, om
    assert ver(m=l - 1)[0] == EINVAL  # needs l points
    assert ver(count=0)[0] == EINVAL and ver(count=(1 << 20) + 1)[0] == EINVAL
    assert ver(ll=8, m=8, count=(1 << 19) + 1)[0] == EINVAL  # count * l > 2^22 with count within its own limit
    assert ver(idx=np.array([1, n // l], dtype=np.uint64))[0] == EINVAL
    bad_ys = base["ys"].copy()
    bad_ys[4 * (2 * l - 1):] = limbs([R])
    assert ver(ys=bad_ys)[0] == EINVAL
    assert ver(rho=limbs([3, 0]))[0] == EINVAL and ver(rho=limbs([R, 4]))[0] == EINVAL
    assert ver() == (0, 1)
