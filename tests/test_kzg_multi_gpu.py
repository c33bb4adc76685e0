"""Multi-point KZG openings over BN254 (csrc/kzg_multi.hip): open, finish and verify, bit-exact
against the integer model tests/kzg_multi_expect.py -- no tolerance anywhere.

Expected points use the trapdoor S of the test SRS (O(len) big-integer work and one g1_mul each), so
they do not depend on the GPU's MSM. Shapes: the division works in blocks of 4096 quotient
coefficients (HS_BLK; len is the quotient's length plus one) and the evaluation in chunks of 16384,
the sizes the lens surround; one case passes 256 blocks, where one thread of the totals' pass takes
more than one block. The weighted sums take 10 inputs per launch (batches 1, 2, 11, 21)."""
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
import kzg_multi_expect as X  # noqa: E402

pytestmark = pytest.mark.gpu
R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R  # the trapdoor
M = 40000       # device SRS: M + 1 points
M_HOST = 4200   # host SRS: M_HOST + 1 points


def horner(c, x):
    y = 0
    for ci in reversed(c):
        y = (y * x + ci) % R
    return y


class World:
    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch
        self.d_srs = torch.empty(8 * (M + 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.srs_create_dev(S, M, self.d_srs.data_ptr())
        torch.cuda.synchronize()
        self.srs = ctx.srs_create(S, M_HOST)
        self.g2s = [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [S])[0]]
        self._polys = {}

    def polys(self, ln, batch, pitch, seed):
        """(limb array of batch * pitch elements, [coefficient lists], [p_b(S)]) -- random canonical
        values, the gaps between polynomials filled too (they must not be read)."""
        key = (ln, batch, pitch, seed)
        if key not in self._polys:
            a = F.random_limbs(batch * pitch, seed)
            ints = F.limbs_to_ints(a)
            polys = [ints[b * pitch:b * pitch + ln] for b in range(batch)]
            self._polys[key] = (a, polys, [horner(p, S) for p in polys])
        return self._polys[key]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

    def mul_g(self, ks):
        """[k]G for every k: commitments of constant polynomials (model scalars to points)"""
        return self.ctx.kzg_commit(self.srs[:1], [[k % R] for k in ks])


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


def expect(polys, vals, pts, sets, gamma, z):
    """(ys, W, W') of the model"""
    ys = [[horner(p, t) if (m >> j) & 1 else 0 for j, t in enumerate(pts)] for p, m in zip(polys, sets)]
    w = X.enc(F.g1_mul(F.G1_GEN, X.h_at(vals, ys, pts, sets, gamma, S)))
    return ys, w, X.expect_finish(polys, pts, sets, gamma, z, S, vals=vals, ys=ys)


def run_dev(ctx, world, d, ln, pitch, batch, pts, sets, gamma, z, d_srs=None, srs_m=M + 1):
    srs = world.d_srs.data_ptr() if d_srs is None else d_srs
    ys, w = ctx.kzg_open_multi_dev(srs, srs_m, d.data_ptr(), ln, pitch, batch, pts, sets, gamma)
    return ys, w, ctx.kzg_open_multi_finish_dev(srs, srs_m, d.data_ptr(), ln, pitch, batch, pts, sets, gamma, z)


def check_dev(ctx, world, ln, batch, pts, sets, gamma, z, seed, pitch=None):
    pitch = pitch or ln
    a, polys, vals = world.polys(ln, batch, pitch, seed)
    got = run_dev(ctx, world, world.dev(a), ln, pitch, batch, pts, sets, gamma, z)
    want = expect(polys, vals, pts, sets, gamma, z)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    return polys, vals, got


# |S| = 3 and 2: len = 2, 3, 4 are |S| - 1 .. |S| + 1; then the block and chunk boundaries
LENS = [1, 2, 3, 4, 4095, 4096, 4097, 4098, 8193, 16383, 16385, 32769]


@pytest.mark.parametrize("ln", LENS)
def test_lens(ctx, world, ln):
    rng = random.Random(ln)
    pts = X.distinct(rng, 3, [S])
    check_dev(ctx, world, ln, 2, pts, [0b111, 0b101], rng.randrange(R), rng.randrange(R), 100 + ln)


def test_more_than_256_blocks(ctx, world):
    """len = 256 * 4096 + 2, batch = 2: the totals' pass takes two blocks per thread. Coefficients of
    64 bits keep the model's cost down; the running values are full-size from the first step on."""
    import torch

    ln, batch = 256 * 4096 + 2, 2
    nrng = np.random.default_rng(5)
    lo = nrng.integers(0, 1 << 63, size=batch * ln, dtype=np.uint64)
    a = np.zeros((batch * ln, 4), dtype=np.uint64)
    a[:, 0] = lo
    ints = lo.tolist()
    polys = [ints[b * ln:(b + 1) * ln] for b in range(batch)]
    d_srs = torch.empty(8 * ln, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs_create_dev(S, ln - 1, d_srs.data_ptr())
    torch.cuda.synchronize()
    rng = random.Random(6)
    pts, sets, gamma, z = X.distinct(rng, 2, [S]), [0b11, 0b01], rng.randrange(R), rng.randrange(R)
    got = run_dev(ctx, world, world.dev(a.reshape(-1)), ln, ln, batch, pts, sets, gamma, z, d_srs.data_ptr(), ln)
    assert got == expect(polys, [horner(p, S) for p in polys], pts, sets, gamma, z)


def set_shapes(npts, rng):
    full = (1 << npts) - 1
    shapes = {"full": [full] * 3, "singletons": [1 << (b % npts) for b in range(4)]}
    if npts > 1:
        own = []
        while len(own) < 4:
            m = rng.randrange(1, full + 1)
            if m not in own or len(own) >= full:
                own.append(m)
        shapes["own"] = own
        shapes["grouped"] = [own[0], own[1], own[0], full, own[1]]  # equal sets at non-adjacent indices
        shapes["unused"] = [m & ~2 or 1 for m in own]  # t_1 lies in no set
    return shapes


@pytest.mark.parametrize("npts", [1, 2, 3, 8, 32])
def test_set_shapes(ctx, world, npts):
    rng = random.Random(300 + npts)
    pts = X.distinct(rng, npts, [S])
    for name, sets in set_shapes(npts, rng).items():
        ln = 4100 if name == "grouped" else 70
        check_dev(ctx, world, ln, len(sets), pts, sets, rng.randrange(R), rng.randrange(R), 400 + npts)


@pytest.mark.parametrize("batch", [1, 2, 11, 21])
def test_batches_on_one_set(ctx, world, batch):
    rng = random.Random(500 + batch)
    pts = X.distinct(rng, 3, [S])
    check_dev(ctx, world, 4097, batch, pts, [0b110] * batch, rng.randrange(R), rng.randrange(R), 500)


def test_thirteen_polynomials_over_five_sets(ctx, world):
    rng = random.Random(513)
    pts = X.distinct(rng, 4, [S])
    kinds = [0b1111, 0b0001, 0b1010, 0b0110, 0b1101]
    sets = [kinds[(b * 3) % 5] if b != 7 else kinds[0] for b in range(13)]
    assert len(set(sets)) == 5
    check_dev(ctx, world, 4099, 13, pts, sets, rng.randrange(R), rng.randrange(R), 513)


def test_pitch_larger_than_len_host_and_dev(ctx, world):
    """pitch > len, the gaps filled with random values, through the host and the _dev forms; the two
    agree with the model and so with each other."""
    ln, batch, pitch = 4099, 3, 4099 + 33
    rng = random.Random(600)
    pts, sets, gamma, z = X.distinct(rng, 3, [S]), [0b011, 0b100, 0b011], rng.randrange(R), rng.randrange(R)
    polys, vals, got = check_dev(ctx, world, ln, batch, pts, sets, gamma, z, 600, pitch=pitch)
    a = world.polys(ln, batch, pitch, 600)[0]
    lib, h = ctx.lib, ctx.h
    import pbf

    ptr = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
    srs = pbf._g1_limbs(world.srs[:ln - 1])
    lp, ls = pbf.ints_to_limbs(pts), np.array(sets, dtype=np.uint64)
    lg, lz = pbf.ints_to_limbs([gamma]), pbf.ints_to_limbs([z])
    ys, w, w2 = np.zeros(4 * batch * 3, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    assert lib.pbf_kzg_open_multi_bn254(h, ptr(srs), ln - 1, ptr(a), ln, pitch, batch, ptr(lp), 3, ptr(ls), ptr(lg),
                                        ptr(ys), ptr(w)) == 0
    assert lib.pbf_kzg_open_multi_finish_bn254(h, ptr(srs), ln - 1, ptr(a), ln, pitch, batch, ptr(lp), 3, ptr(ls),
                                               ptr(lg), ptr(lz), ptr(w2)) == 0
    v = pbf.limbs_to_ints(ys)
    assert [v[3 * b:3 * b + 3] for b in range(batch)] == got[0]
    assert ctx._points(w)[0] == got[1] and ctx._points(w2)[0] == got[2]


def _poly_with_root(rng, ln, a):
    g = [rng.randrange(R) for _ in range(ln - 1)]
    return X.poly_mul_linear(g, a)


def test_special_values(ctx, world):
    """z in T, z = 0, z a root of a polynomial; gamma = 0 and 1; a point t = 0; the zero polynomial;
    W and W' the identity at len = 1."""
    rng = random.Random(700)
    ln = 33
    srs = world.srs[:ln - 1]
    root = rng.randrange(R)
    polys = [_poly_with_root(rng, ln, root), [rng.randrange(R) for _ in range(ln)], [0] * ln]
    pts = [0] + X.distinct(rng, 2, [S, 0])
    sets = [0b011, 0b110, 0b101]
    vals = [horner(p, S) for p in polys]
    for gamma, z in ((0, pts[1]), (1, 0), (rng.randrange(R), root), (rng.randrange(R), pts[0]), (0, 0)):
        ys, w = ctx.kzg_open_multi(srs, polys, pts, sets, gamma)
        w2 = ctx.kzg_open_multi_finish(srs, polys, pts, sets, gamma, z)
        assert (ys, w, w2) == expect(polys, vals, pts, sets, gamma, z), (gamma, z)
        assert ys[2] == [0, 0, 0]
    # every polynomial zero: both proofs are the identity
    zero = [[0] * ln] * 2
    assert ctx.kzg_open_multi(srs, zero, pts, [0b111, 0b001], 5) == ([[0] * 3] * 2, (0, 0))
    assert ctx.kzg_open_multi_finish(srs, zero, pts, [0b111, 0b001], 5, 9) == (0, 0)
    # len = 1: constants, empty quotients, and the SRS is not read
    const = [[7], [rng.randrange(R)]]
    ys, w = ctx.kzg_open_multi([], const, pts, [0b101, 0b010], 3)
    assert ys == [[7, 0, 7], [0, const[1][0], 0]] and w == (0, 0)
    assert ctx.kzg_open_multi_finish([], const, pts, [0b101, 0b010], 3, 11) == (0, 0)


def test_one_point_is_the_plain_opening(ctx, world):
    """npts = 1, every set {t_0}: y and W are what pbf_kzg_open_bn254 returns for the weights gamma^b,
    bit for bit (and W' = W: with one point the second proof carries nothing new)."""
    rng = random.Random(800)
    ln, batch = 4100, 4
    a, polys, _ = world.polys(ln, batch, ln, 800)
    t, gamma = rng.randrange(R), rng.randrange(R)
    d = world.dev(a)
    ys, w = ctx.kzg_open_multi_dev(world.d_srs.data_ptr(), M + 1, d.data_ptr(), ln, ln, batch, [t], [1] * batch, gamma)
    pys, pw = ctx.kzg_open_dev(world.d_srs.data_ptr(), M + 1, d.data_ptr(), ln, ln, batch, t, X.gamma_pows(gamma, batch))
    assert [r[0] for r in ys] == pys and w == pw
    w2 = ctx.kzg_open_multi_finish_dev(world.d_srs.data_ptr(), M + 1, d.data_ptr(), ln, ln, batch, [t], [1] * batch,
                                       gamma, rng.randrange(R))
    assert w2 == w


def test_plain_opening_unchanged_by_a_multi_call(ctx, world):
    """A multi call between two plain openings on one context does not change what the second returns."""
    rng = random.Random(810)
    ln, batch = 4100, 3
    a, polys, _ = world.polys(ln, batch, ln, 810)
    d = world.dev(a)
    z, weights = rng.randrange(R), [rng.randrange(R) for _ in range(batch)]
    srs = world.d_srs.data_ptr()
    first = ctx.kzg_open_dev(srs, M + 1, d.data_ptr(), ln, ln, batch, z, weights)
    pts = X.distinct(rng, 3, [S])
    ctx.kzg_open_multi_dev(srs, M + 1, d.data_ptr(), ln, ln, batch, pts, [7, 5, 2], 3)
    ctx.kzg_open_multi_finish_dev(srs, M + 1, d.data_ptr(), ln, ln, batch, pts, [7, 5, 2], 3, 4)
    assert ctx.kzg_open_dev(srs, M + 1, d.data_ptr(), ln, ln, batch, z, weights) == first


# ---------------------------------------------------------------- verify
def test_verify_accepts_what_open_and_finish_return(ctx, world):
    rng = random.Random(900)
    ln, batch, sets = 70, 3, [0b110, 0b011, 0b110]
    openings = []
    for i in range(3):
        polys = [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]
        pts, gamma, z = X.distinct(rng, 3, [S]), rng.randrange(R), rng.randrange(R)
        commits = ctx.kzg_commit(world.srs[:ln], polys)
        ys, w = ctx.kzg_open_multi(world.srs[:ln - 1], polys, pts, sets, gamma)
        w2 = ctx.kzg_open_multi_finish(world.srs[:ln - 1], polys, pts, sets, gamma, z)
        openings.append((commits, pts, ys, gamma, z, w, w2))
    assert ctx.kzg_verify_multi(world.g2s, sets, openings[:1], [1])
    assert ctx.kzg_verify_multi(world.g2s, sets, openings, [rng.randrange(1, R) for _ in range(3)])


class Made:
    """300 model-made openings of len = 4, batch = 2, npts = 3: scalars from the model, points from
    one commitment call over constants"""

    def __init__(self, world):
        rng = random.Random(910)
        self.sets = [0b101, 0b110]
        rows, ks = [], []
        for _ in range(300):
            polys = [[rng.randrange(R) for _ in range(4)] for _ in range(2)]
            pts, gamma, z = X.distinct(rng, 3, [S]), rng.randrange(R), rng.randrange(R)
            vals = [horner(p, S) for p in polys]
            ys = X.expect_ys(polys, pts, self.sets)
            rows.append((pts, ys, gamma, z))
            ks += vals + [X.h_at(vals, ys, pts, self.sets, gamma, S), X.w2_scalar(vals, ys, pts, self.sets, gamma, z, S)]
        g = world.mul_g(ks)
        self.openings = [(g[4 * i:4 * i + 2], r[0], r[1], r[2], r[3], g[4 * i + 2], g[4 * i + 3])
                         for i, r in enumerate(rows)]
        self.rhos = [rng.randrange(1, R) for _ in range(300)]


@pytest.fixture(scope="module")
def made(world):
    return Made(world)


@pytest.mark.parametrize("count", [255, 256, 257, 300])
def test_verify_counts(ctx, world, made, count):
    """the 256-lane block boundaries of the verifier's kernels"""
    assert ctx.kzg_verify_multi(world.g2s, made.sets, made.openings[:count], made.rhos[:count])
    bad = list(made.openings[:count])
    o = bad[count - 1]
    bad[count - 1] = (o[0], o[1], [o[2][0], [o[2][1][0], (o[2][1][1] + 1) % R, o[2][1][2]]], o[3], o[4], o[5], o[6])
    assert not ctx.kzg_verify_multi(world.g2s, made.sets, bad, made.rhos[:count])


def test_verify_rejections(ctx, world, made):
    sets, ops, rhos = made.sets, made.openings[:3], made.rhos[:3]
    ver = lambda o, s=sets: ctx.kzg_verify_multi(world.g2s, s, o, rhos)  # noqa: E731
    assert ver(ops)

    def with_(i, **kw):
        names = ["commits", "pts", "ys", "gamma", "z", "w", "w2"]
        o = list(ops[i])
        for k, v in kw.items():
            o[names.index(k)] = v
        return ops[:i] + [tuple(o)] + ops[i + 1:]

    c, pts, ys, gamma, z, w, w2 = ops[1]
    # garbage in y outside the sets is not read: set 0 = {t_0, t_2}, set 1 = {t_1, t_2}
    assert ver(with_(1, ys=[[ys[0][0], R + 5, ys[0][2]], [(1 << 256) - 1, ys[1][1], ys[1][2]]]))
    assert not ver(with_(1, ys=[[ys[0][0], 0, (ys[0][2] + 1) % R], ys[1]]))       # one y changed
    assert not ver(with_(1, w=w2, w2=w))                                           # W and W' swapped
    assert not ver(with_(1, gamma=(gamma + 1) % R))
    assert not ver(with_(1, z=(z + 1) % R))
    assert not ver(ops, [0b101, 0b111])                                            # one wrong mask bit
    assert not ver(with_(1, commits=[c[0], ops[0][0][1]]))                         # one commitment replaced
    assert not ver(with_(1, w2=(w2[0], (w2[1] + 1) % F.Q)))                        # an off-curve W'
    assert not ver(with_(2, w=(F.Q, 0)))                                           # not canonical


def test_rho_contract(ctx, world, made):
    """With equal rho two errors that cancel pass; with distinct rho they do not. The library reads
    no randomness: choosing rho unpredictably, after the openings, is the caller's part."""
    sets = made.sets
    c, pts, ys, gamma, z, w, w2 = made.openings[0]
    d = 12345
    up = [[(ys[0][0] + d) % R, 0, ys[0][2]], ys[1]]
    down = [[(ys[0][0] - d) % R, 0, ys[0][2]], ys[1]]
    pair = [(c, pts, up, gamma, z, w, w2), (c, pts, down, gamma, z, w, w2)]
    assert ctx.kzg_verify_multi(world.g2s, sets, pair, [1, 1])
    assert ctx.kzg_verify_multi(world.g2s, sets, pair, [77, 77])
    assert not ctx.kzg_verify_multi(world.g2s, sets, pair, [1, 2])
    assert not ctx.kzg_verify_multi(world.g2s, sets, pair[:1], [1])


# ---------------------------------------------------------------- errors
def test_errors(ctx, world, made):
    """Every argument error returns PBF_EINVAL, leaves pbf_last_error set and writes nothing."""
    import pbf

    lib, h = ctx.lib, ctx.h
    ptr = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
    L = pbf.ints_to_limbs
    rng = random.Random(990)
    srs = pbf._g1_limbs(world.srs[:8])
    polys = L([rng.randrange(R) for _ in range(8)])
    pts, eq, big_pts = L([1, 2, 3]), L([1, 2, 1]), L([1, R, 3])
    sets, zero_set, high_set = (np.array(v, dtype=np.uint64) for v in ([7, 5], [7, 0], [7, 8]))
    one, big = L([1]), L([R])
    SENT = 0xA5A5A5A5A5A5A5A5
    out_y, out_w = np.full(4 * 2 * 3, SENT, np.uint64), np.full(8, SENT, np.uint64)
    d = world.dev(polys)
    d_srs = world.d_srs.data_ptr()
    vp = ctypes.c_void_p

    def opn(srs_=srs, m=8, p=polys, ln=4, pitch=4, batch=2, t=pts, npts=3, s=sets, g=one, y=out_y, w=out_w):
        return lib.pbf_kzg_open_multi_bn254(h, ptr(srs_) if srs_ is not None else None, m,
                                            ptr(p) if p is not None else None, ln, pitch, batch,
                                            ptr(t) if t is not None else None, npts, ptr(s) if s is not None else None,
                                            ptr(g) if g is not None else None, ptr(y) if y is not None else None,
                                            ptr(w) if w is not None else None)

    def fin(z=one, w=out_w, **kw):
        a = dict(srs_=srs, m=8, p=polys, ln=4, pitch=4, batch=2, t=pts, npts=3, s=sets, g=one)
        a.update(kw)
        return lib.pbf_kzg_open_multi_finish_bn254(h, ptr(a["srs_"]), a["m"], ptr(a["p"]), a["ln"], a["pitch"],
                                                   a["batch"], ptr(a["t"]), a["npts"], ptr(a["s"]), ptr(a["g"]),
                                                   ptr(z) if z is not None else None, ptr(w) if w is not None else None)

    assert opn() == 0 and out_y[0] != SENT  # the valid call the others are one step away from
    out_y[:], out_w[:] = SENT, SENT
    many = L(list(range(1, 34)))
    bad = []
    for f in (opn, fin):
        calls = [dict(ln=0), dict(batch=0), dict(batch=(1 << 16) + 1), dict(pitch=3), dict(m=2),       # open's own
                 dict(npts=0), dict(t=many, npts=33), dict(t=eq), dict(t=big_pts),
                 dict(s=zero_set), dict(s=high_set), dict(g=big)]
        calls += [dict(srs_=None), dict(p=None), dict(t=None), dict(s=None), dict(g=None), dict(y=None),
                  dict(w=None)] if f is opn else \
            [dict(z=None), dict(w=None), dict(z=big)]
        for kw in calls:
            bad.append((kw, f(**kw)))
            assert lib.pbf_last_error(), kw
    assert [b for b in bad if b[1] != pbf.PBF_EINVAL] == []
    assert (out_y == SENT).all() and (out_w == SENT).all()
    # the _dev forms check the same things before touching the device pointers
    with pytest.raises(pbf.PbfError) as e:
        ctx.kzg_open_multi_dev(d_srs, M + 1, d.data_ptr(), 4, 3, 2, [1, 2, 3], [7, 5], 1)
    assert e.value.code == pbf.PBF_EINVAL
    with pytest.raises(pbf.PbfError) as e:
        ctx.kzg_open_multi_finish_dev(d_srs, M + 1, d.data_ptr(), 4, 4, 2, [1, 2, 2], [7, 5], 1, 1)
    assert e.value.code == pbf.PBF_EINVAL
    with pytest.raises(pbf.PbfError) as e:
        ctx.kzg_open_multi_dev(d_srs, 2, d.data_ptr(), 4, 4, 2, [1, 2, 3], [7, 5], 1)
    assert e.value.code == pbf.PBF_EINVAL

    # the verifier
    sets2, ops = made.sets, made.openings[:2]

    def ver(ops_=ops, rhos=(1, 2), s=sets2):
        with pytest.raises(pbf.PbfError) as e:
            ctx.kzg_verify_multi(world.g2s, s, ops_, list(rhos))
        return e.value.code

    c, t, ys, gamma, z, w, w2 = ops[1]
    chg = lambda i, v: [ops[0], tuple(v if k == i else x for k, x in enumerate(ops[1]))]  # noqa: E731
    codes = [ver(rhos=(1, 0)), ver(rhos=(R, 1)), ver(chg(1, [t[0], t[1], t[0]])), ver(chg(1, [t[0], R, t[2]])),
             ver(chg(3, R)), ver(chg(4, R + 1)), ver(chg(2, [[R, 0, ys[0][2]], ys[1]])),
             ver(s=[0b101, 0]), ver(s=[0b101, 0b1010]), ver([], ())]
    assert codes == [pbf.PBF_EINVAL] * len(codes), codes
    ok = ctypes.c_int(-7)
    g2 = pbf._g2_limbs(world.g2s)
    z8, z4, s1 = np.zeros(8 * 4, np.uint64), L([1, 2, 3, 4]), np.array([1], dtype=np.uint64)
    raw = lambda count, batch, npts, okp: lib.pbf_kzg_verify_multi_bn254(  # noqa: E731
        h, ptr(g2), count, batch, npts, ptr(s1), ptr(z8), ptr(z4), ptr(z4), ptr(z4), ptr(z4), ptr(z8), ptr(z8),
        ptr(z4), okp)
    # count = 0, count * batch > 2^20 (checked before anything is read), npts = 0 and 33, a null ok
    rcs = [raw(0, 1, 1, ctypes.byref(ok)), raw((1 << 20) + 1, 1, 1, ctypes.byref(ok)),
           raw((1 << 5) + 1, 1 << 15, 1, ctypes.byref(ok)), raw(1, 1, 0, ctypes.byref(ok)),
           raw(1, 1, 33, ctypes.byref(ok)), raw(1, 1, 1, None)]
    assert rcs == [pbf.PBF_EINVAL] * len(rcs), rcs
    assert ok.value == -7
    # and the next valid calls are right
    assert ctx.kzg_verify_multi(world.g2s, sets2, ops, [3, 4])
    assert opn() == 0 and out_y[0] != SENT
