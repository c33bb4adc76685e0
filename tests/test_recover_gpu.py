"""Recovery from cells (csrc/kzg_recover.hip pbf_kzg_recover_cells_bn254*), bit-exact: no tolerance
anywhere. The expected polynomial is the one the cells were made from and the expected out_y its
cell values (tests/fk20_cells_expect.py cell_values); for inconsistent input the interpolant of
tests/recover_expect.py. Input cells come from the Python restatement up to n = 2^14 and from the
library's own Fr NTT above that, compared as device tensors.

Shapes. Every (n, l) with l <= n <= 64 and six known sets each. (512, 2) .. (2^14, 64) walk the
transforms' boundaries, (2^18, 64) and (2^19, 64) are two and three passes at ntt256.maxr = 9, and
k = 2^13 .. 2^16 stage the roots of k_rec_zvals through LDS over many tiles; k = 2^16 is the
supported maximum."""
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
import fk20_cells_expect as C  # noqa: E402
import recover_expect as E  # noqa: E402

pytestmark = pytest.mark.gpu
R = F.R
EINVAL = 1


def omega_of(n):
    return F.root_of_unity(n)


def random_polys(rng, batch, ln):
    return [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]


def min_count(ln, l):
    return (ln + l - 1) // l


def shuffled(rng, idx):
    idx = list(idx)
    rng.shuffle(idx)
    return idx


class Dev:
    """Device buffers and one call of the _dev form."""

    def __init__(self):
        import torch

        self.torch = torch

    def limbs(self, values):
        return self.torch.from_numpy(F.ints_to_limbs(values).view(np.int64)).cuda()

    def ints(self, t):
        return F.limbs_to_ints(t.cpu().numpy().view(np.uint64))

    def call(self, ctx, n, l, ln, idx, d_cells, batch, pitch=None, with_y=True, side_stream=False):
        """(d_polys [batch, pitch, 4], d_y [batch, k, l, 4] or None, consistent as a list); the outputs
        were filled with -1, and whatever the call must not write still is."""
        torch = self.torch
        pitch = pitch or ln
        d_p = torch.full((batch, pitch, 4), -1, dtype=torch.int64, device="cuda")
        d_y = torch.full((batch, n // l, l, 4), -1, dtype=torch.int64, device="cuda")
        d_f = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream() if side_stream else None
        ctx.kzg_recover_cells_dev(omega_of(n), n, l, ln, idx, d_cells.data_ptr(), batch, d_p.data_ptr(), pitch,
                                  d_y.data_ptr() if with_y else 0, d_f.data_ptr(), stream=st.cuda_stream if st else 0)
        if st:
            st.synchronize()
        torch.cuda.synchronize()
        assert bool((d_p[:, ln:] == -1).all())  # the gap words
        if not with_y:
            assert bool((d_y == -1).all())
        return d_p, (d_y if with_y else None), d_f.cpu().tolist()

    def recover(self, ctx, n, l, ln, idx, cells, **kw):
        """The same from and to Python integers: cells[b][j] lists of l values ->
        (polys[b], ys[b][i] or None, consistent)."""
        batch, k = len(cells), n // l
        d_p, d_y, flags = self.call(ctx, n, l, ln, idx, self.limbs([v for c in cells for cell in c for v in cell]), batch, **kw)
        p = self.ints(d_p[:, :ln].contiguous())
        polys = [p[b * ln:(b + 1) * ln] for b in range(batch)]
        if d_y is None:
            return polys, None, flags
        v = self.ints(d_y)
        return polys, [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)], flags


@pytest.fixture(scope="module")
def dev():
    return Dev()


def check(dev, ctx, n, l, polys, idx, **kw):
    """One call on the cells idx of polys against the polynomials themselves."""
    omega, ln = omega_of(n), len(polys[0])
    want_y = [C.cell_values(p, n, l, omega) for p in polys]
    cells = [[list(y[i]) for i in idx] for y in want_y]
    got = dev.recover(ctx, n, l, ln, idx, cells, **kw)
    assert got[0] == polys, (n, l, idx)
    assert got[1] is None or got[1] == want_y, (n, l, idx)
    assert got[2] == [1] * len(polys)
    return got


# ---------------------------------------------------------------- every shape up to n = 64
POW2 = [1, 2, 4, 8, 16, 32, 64]
SHAPES = [(n, l) for n in POW2 for l in POW2 if l <= n]


def known_sets(rng, k, count):
    sets = [rng.sample(range(k), count), range(count), range(k - count, k), range(k)]
    if k >= 2:
        sets += [range(0, k, 2), range(1, k, 2)]
    return [shuffled(rng, s) for s in sets]


@pytest.mark.parametrize("n,l", SHAPES)
def test_every_shape(ctx, dev, n, l):
    rng = random.Random(100 * n + l)
    ln, k = max(1, n // 2), n // l
    polys = random_polys(rng, 2, ln)
    for idx in known_sets(rng, k, min_count(ln, l)):
        check(dev, ctx, n, l, polys, idx)


# ---------------------------------------------------------------- lengths
@pytest.mark.parametrize("ln", [1, 8, 9, 31, 32, 33, 63, 64])
def test_lengths(ctx, dev, ln):
    n, l, k = 64, 8, 8
    rng = random.Random(ln)
    polys = random_polys(rng, 2, ln)
    check(dev, ctx, n, l, polys, shuffled(rng, rng.sample(range(k), min_count(ln, l))))  # len = 64 needs all cells
    check(dev, ctx, n, l, polys, shuffled(rng, range(k)))


def test_zero_polynomial_and_a_zero_cell(ctx, dev):
    n, l, k, ln = 64, 8, 8, 32
    rng = random.Random(5)
    check(dev, ctx, n, l, [[0] * ln, random_polys(rng, 1, ln)[0]], [6, 1, 3, 4])
    # p = (x^l - c_i) q is zero on the whole of cell i, which is known
    i = 3
    q = random_polys(rng, 1, ln - l)[0]
    ci = pow(omega_of(n), i * l, R)
    p = [((q[j - l] if j >= l else 0) - ci * (q[j] if j < ln - l else 0)) % R for j in range(ln)]
    assert C.cell_values(p, n, l, omega_of(n))[i] == [0] * l
    check(dev, ctx, n, l, [p], [5, i, 0, 7])
    check(dev, ctx, n, l, [p], [i, 2, 4, 6, 1])


# ---------------------------------------------------------------- transform boundaries
@pytest.mark.parametrize("n,l", [(512, 2), (1024, 2), (1 << 11, 64), (1 << 12, 64), (1 << 13, 64), (1 << 14, 64)])
def test_transform_boundaries(ctx, dev, n, l):
    rng = random.Random(7 * n + l)
    k = n // l
    check(dev, ctx, n, l, random_polys(rng, 1, n // 2), shuffled(rng, rng.sample(range(k), k // 2)))


@pytest.mark.parametrize("n,l", [(1 << 18, 64), (1 << 19, 64), (1 << 16, 1)])
def test_large_sizes(ctx, dev, n, l):
    """Cells from the library's own forward transform; everything compared on the device."""
    torch = dev.torch
    rng = random.Random(n + l)
    k, ln = n // l, n // 2
    idx = shuffled(rng, rng.sample(range(k), k // 2))
    d_in = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_in[:ln] = torch.from_numpy(F.random_limbs(ln, n + l).view(np.int64).reshape(ln, 4)).cuda()
    d_ev = torch.empty_like(d_in)
    torch.cuda.synchronize()
    ctx.ntt_fr_batch_dev(omega_of(n), d_in.data_ptr(), d_ev.data_ptr(), n, 1)
    torch.cuda.synchronize()
    want_y = d_ev.view(l, k, 4).permute(1, 0, 2).contiguous()  # [i][t] = y[i + k t]
    d_cells = want_y[torch.tensor(idx, device="cuda")].contiguous()
    d_p, d_y, flags = dev.call(ctx, n, l, ln, idx, d_cells, 1)
    assert flags == [1]
    assert torch.equal(d_p[0], d_in[:ln])
    assert torch.equal(d_y[0], want_y)


def test_limbs_of_32_bits(dev):
    """Option ntt256.l29 = 0: the transforms on 32-bit limbs, equal to the default bit for bit."""
    import pbf

    n, l, k = 1024, 64, 16
    rng = random.Random(29)
    polys = random_polys(rng, 2, n // 2)
    c = pbf.Context(0, options={"ntt256.l29": "0"})
    try:
        check(dev, c, n, l, polys, shuffled(rng, rng.sample(range(k), k // 2)))
    finally:
        c.close()


# ---------------------------------------------------------------- batches, pitch, call forms
@pytest.mark.parametrize("batch", [1, 6, 70])
def test_batches_and_pitch(ctx, dev, batch):
    n, l, k, ln = 64, 8, 8, 29
    rng = random.Random(batch)
    polys = random_polys(rng, batch, ln)
    idx = shuffled(rng, rng.sample(range(k), 5))
    a = check(dev, ctx, n, l, polys, idx)
    assert check(dev, ctx, n, l, polys, idx, pitch=ln + 5) == a
    for b in sorted({0, batch // 2, batch - 1}):  # the batch equals single calls
        assert check(dev, ctx, n, l, [polys[b]], idx) == ([a[0][b]], [a[1][b]], [1])


def test_no_state_between_calls(ctx, dev):
    """One context, one (n, l), three different missing sets, then the first again: nothing about
    the missing set may outlive a call."""
    n, l, ln = 64, 8, 32
    rng = random.Random(3)
    polys = random_polys(rng, 2, ln)
    for idx in ([0, 1, 2, 3], [7, 5, 3, 1], [4, 0, 6, 2, 5], [0, 1, 2, 3]):
        check(dev, ctx, n, l, polys, idx)


def test_without_y_and_on_a_side_stream(ctx, dev):
    n, l, ln = 64, 8, 32
    rng = random.Random(11)
    polys = random_polys(rng, 3, ln)
    idx = [6, 2, 7, 0]
    a = check(dev, ctx, n, l, polys, idx)
    assert check(dev, ctx, n, l, polys, idx, with_y=False) == (a[0], None, a[2])
    assert check(dev, ctx, n, l, polys, idx, side_stream=True) == a


# ---------------------------------------------------------------- consistency
def redundant(rng):
    n, l, ln, idx = 64, 8, 29, [6, 0, 3, 5, 2]
    polys = random_polys(rng, 3, ln)
    ys = [C.cell_values(p, n, l, omega_of(n)) for p in polys]
    return n, l, ln, idx, polys, ys, [[list(y[i]) for i in idx] for y in ys]


def check_one_bad(dev, ctx, n, l, ln, idx, polys, ys, cells):
    """Polynomial 1's cells were altered: it alone is flagged, and its outputs are the first len
    coefficients of the interpolant and their cells, canonical."""
    got_p, got_y, flags = dev.recover(ctx, n, l, ln, idx, cells)
    assert flags == [1, 0, 1]
    assert (got_p[0], got_p[2]) == (polys[0], polys[2]) and (got_y[0], got_y[2]) == (ys[0], ys[2])
    want = E.recover(cells[1], idx, n, l, ln, omega_of(n))
    assert want[2] == 0 and (got_p[1], got_y[1]) == want[:2]
    assert all(v < R for v in got_p[1]) and all(v < R for c in got_y[1] for v in c)


@pytest.mark.parametrize("t", [0, 7])
def test_one_changed_value(ctx, dev, t):
    n, l, ln, idx, polys, ys, cells = redundant(random.Random(40 + t))
    cells[1][2][t] = (cells[1][2][t] + 1) % R
    check_one_bad(dev, ctx, n, l, ln, idx, polys, ys, cells)


def test_a_value_swapped_between_two_cells(ctx, dev):
    n, l, ln, idx, polys, ys, cells = redundant(random.Random(50))
    cells[1][0][3], cells[1][4][3] = cells[1][4][3], cells[1][0][3]
    check_one_bad(dev, ctx, n, l, ln, idx, polys, ys, cells)


@pytest.mark.parametrize("n,l,count", [(64, 8, 4), (16, 1, 8), (16, 16, 1)])
def test_arbitrary_values_are_consistent_without_redundancy(ctx, dev, n, l, count):
    """count * l == len: any values are the cells of a polynomial of len coefficients."""
    rng = random.Random(n + l)
    ln, k = count * l, n // l
    idx = shuffled(rng, rng.sample(range(k), count))
    cells = [[[rng.randrange(R) for _ in range(l)] for _ in idx] for _ in range(2)]
    polys, ys, flags = dev.recover(ctx, n, l, ln, idx, cells)
    assert flags == [1, 1]
    for b in range(2):
        assert [ys[b][i] for i in idx] == cells[b]
        assert ys[b] == C.cell_values(polys[b], n, l, omega_of(n))
        assert (polys[b], ys[b], 1) == E.recover(cells[b], idx, n, l, ln, omega_of(n))


# ---------------------------------------------------------------- with the cell proofs
@pytest.mark.parametrize("n,l", [(64, 8), (1024, 64)])
def test_recovered_cells_are_proven_and_verified(ctx, dev, n, l):
    """Open two polynomials in cells, drop a random half of the cells, recover, open the recovered
    coefficients: every proof equals the original's word for word, and the verifier accepts the
    cells that were missing with those proofs."""
    from test_fk20_cells_gpu import World, omega2_of

    torch = dev.torch
    world = World(ctx)
    rng = random.Random(n + l)
    k, ln, omega2 = n // l, n // 2, omega2_of(n)
    assert pow(omega2, 2, R) == omega_of(n)
    polys = random_polys(rng, 2, ln)
    opened = [world.open_cells(ctx, n, l, [p], [1]) for p in polys]
    idx = shuffled(rng, rng.sample(range(k), k // 2))
    missing = [i for i in range(k) if i not in idx]
    cells = [[list(ys[0][i]) for i in idx] for ys, _ in opened]
    d_p, d_y, flags = dev.call(ctx, n, l, ln, idx, dev.limbs([v for c in cells for cell in c for v in cell]), 2)
    assert flags == [1, 1]
    x = world.xext(ctx, n, l)
    entries = []
    for b in range(2):
        d_w = torch.full((8 * k,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.kzg_open_cells_dev(x.data_ptr(), n, l, omega2, d_p[b].data_ptr(), ln, ln, 1, [1], 0, d_w.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(d_w, opened[b][1])
        ws, commit = world.points(d_w), world.commit(polys[b])
        got_y = dev.ints(d_y[b])
        entries += [(commit, i, got_y[i * l:(i + 1) * l], ws[i]) for i in missing]
    rhos = [rng.randrange(1, R) for _ in entries]
    assert ctx.kzg_verify_cells(world.g2s(l), world.host_srs(l), omega_of(n), n, l, entries, rhos)


# ---------------------------------------------------------------- the host form
def test_host_form(ctx):
    n, l, ln, k = 32, 4, 14, 8
    rng = random.Random(12)
    omega = omega_of(n)
    polys = random_polys(rng, 3, ln)
    idx = [5, 0, 7, 2]
    want_y = [C.cell_values(p, n, l, omega) for p in polys]
    cells = [[list(y[i]) for i in idx] for y in want_y]
    assert ctx.kzg_recover_cells(omega, n, l, ln, idx, cells) == (polys, want_y, [1, 1, 1])
    assert ctx.kzg_recover_cells(omega, n, l, ln, idx, cells, pitch=ln + 3) == (polys, want_y, [1, 1, 1])
    assert ctx.kzg_recover_cells(omega, n, l, ln, idx, cells, with_y=False) == (polys, None, [1, 1, 1])
    cells[2][1][0] = (cells[2][1][0] + 1) % R
    got = ctx.kzg_recover_cells(omega, n, l, ln, idx, cells)
    assert got[2] == [1, 1, 0] and got[0][:2] == polys[:2] and got[1][:2] == want_y[:2]
    assert (got[0][2], got[1][2], 0) == E.recover(cells[2], idx, n, l, ln, omega)
    assert ctx.kzg_recover_cells(1, 1, 1, 1, [0], [[[5]], [[6]]]) == ([[5], [6]], [[[5]], [[6]]], [1, 1])


# ---------------------------------------------------------------- errors
def test_errors(ctx, dev):
    import pbf

    torch = dev.torch
    lib, h = ctx.lib, ctx.h
    n, l, ln, count, batch = 16, 4, 8, 3, 2
    k = n // l
    vp = ctypes.c_void_p
    w = lambda v: pbf._ptr(pbf.ints_to_limbs([v]))  # noqa: E731
    ix = lambda v: pbf._ptr(np.array(v, dtype=np.uint64))  # noqa: E731
    om, idx = omega_of(n), [3, 0, 2]
    polys = random_polys(random.Random(1), batch, ln)
    flat = [v for p in polys for i in idx for v in C.cell_values(p, n, l, om)[i]]
    d_c = dev.limbs(flat)
    d_p = torch.full((4 * batch * (ln + 1),), -1, dtype=torch.int64, device="cuda")
    d_y = torch.full((4 * batch * n,), -1, dtype=torch.int64, device="cuda")
    d_f = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def rec(ctxh=h, o=om, nn=n, ll=l, le=ln, cnt=count, ci=idx, c=vp(d_c.data_ptr()), b=batch, p=vp(d_p.data_ptr()),
            pitch=ln, y=vp(d_y.data_ptr()), f=vp(d_f.data_ptr())):
        return lib.pbf_kzg_recover_cells_bn254_dev(ctxh, w(o) if o is not None else None, nn, ll, le, cnt,
                                                   ix(ci) if ci is not None else None, c, b, p, pitch, y, f, None)

    assert rec(ctxh=None) == EINVAL and rec(o=None) == EINVAL and rec(ci=None) == EINVAL
    assert rec(c=None) == EINVAL and rec(p=None) == EINVAL and rec(f=None) == EINVAL
    for nn in (0, 3, 12, 1 << 28, 1 << 40):
        assert rec(nn=nn, o=omega_of(nn) if nn in (1 << 28,) else om) == EINVAL, nn
    for ll in (0, 3, 6, 2 * n, 1 << 40):
        assert rec(ll=ll) == EINVAL, ll
    big = 1 << 17  # k above 2^16
    assert rec(nn=big, ll=1, o=omega_of(big), le=4, cnt=4) == EINVAL
    for o in (omega_of(2 * n), omega_of(n // 2), 0, 1, R, R + om):
        assert rec(o=o) == EINVAL, o
    assert rec(le=0) == EINVAL and rec(le=n + 1, pitch=n + 1) == EINVAL
    assert rec(cnt=0, ci=[]) == EINVAL and rec(cnt=k + 1, ci=[0, 1, 2, 3, 0]) == EINVAL
    assert rec(le=count * l + 1, pitch=count * l + 1) == EINVAL  # count * l = len - 1
    assert rec(ci=[3, k, 2]) == EINVAL and rec(ci=[3, 0, 3]) == EINVAL  # out of range, repeated
    assert rec(b=0) == EINVAL and rec(b=(1 << 16) + 1) == EINVAL
    assert rec(pitch=ln - 1) == EINVAL
    # the host form: a value that is not canonical
    bad = pbf.ints_to_limbs(flat)
    bad[4 * 5:4 * 6] = pbf.ints_to_limbs([R])
    out_p = np.zeros(4 * batch * ln, dtype=np.uint64)
    out_y = np.zeros(4 * batch * n, dtype=np.uint64)
    out_f = np.full(batch, -1, dtype=np.int32)
    fp = out_f.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def host(c):
        return lib.pbf_kzg_recover_cells_bn254(h, w(om), n, l, ln, count, ix(idx), pbf._ptr(c), batch, pbf._ptr(out_p), ln,
                                               pbf._ptr(out_y), fp)

    assert host(bad) == EINVAL
    # nothing was enqueued or written
    torch.cuda.synchronize()
    assert not out_p.any() and not out_y.any() and (out_f == -1).all()
    assert bool((d_p == -1).all()) and bool((d_y == -1).all()) and bool((d_f == -1).all())
    # and the same arguments, valid, succeed
    assert rec() == 0 and rec(y=None) == 0 and rec(pitch=ln + 1) == 0 and host(pbf.ints_to_limbs(flat)) == 0
    torch.cuda.synchronize()
    assert d_f.cpu().tolist() == [1, 1] and out_f.tolist() == [1, 1]
    assert F.limbs_to_ints(out_p) == [v for p in polys for v in p]
    got = dev.ints(d_p.view(batch, ln + 1, 4)[:, :ln].contiguous())
    assert got == [v for p in polys for v in p]
