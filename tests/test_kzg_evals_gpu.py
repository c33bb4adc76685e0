"""KZG in evaluation form (csrc/kzg_evals.hip pbf_kzg_open_evals_bn254*, commit against the Lagrange
SRS of csrc/g1_ntt.hip), bit-exact: no tolerance anywhere.

Expected values use the trapdoor S of the test SRS, as tests/test_kzg_gpu.py: commit(p) = [p(S)]G,
y_b = p_b(z), W = [(sum_b w_b (p_b(S) - y_b)) / (S - z)]G, and W must also equal, word for word,
what kzg_open returns for the coefficient forms. Polynomials are drawn as coefficients; their
evaluations come from the oracle's Fr transform.

Shapes. The new kernels work in workgroups of 256 elements (n = 128, 256, 512: below, one, two) and
sum their per-workgroup partial results in one workgroup of 256 lanes (256 partial sums at
n = 2^16, 512 at 2^17). The batch inversion works in chunks of 64 x 32 elements: n = 2048 is one chunk,
4096 two, and k = 2047 / 2048 are the last element of the first and the first of the second. The
linear combination takes 10 inputs, then 9 more (batches 10, 11, 19, 20) and the dot-product
kernel g = 8 polynomials per launch (batches 7, 8, 9)."""
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
import kzg_evals_expect as E  # noqa: E402

pytestmark = pytest.mark.gpu
R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R  # the trapdoor
M = 1 << 17      # device SRS: M + 1 points
M_HOST = 4096    # host SRS and host Lagrange SRS up to this size


def enc(p):
    return (0, 0) if p is None else p


def inv(a):
    return pow(a % R, R - 2, R)


class World:
    def __init__(self, ctx):
        import torch

        self.ctx, self.torch = ctx, torch
        self.d_srs = torch.empty(8 * (M + 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.srs_create_dev(S, M, self.d_srs.data_ptr())
        torch.cuda.synchronize()
        self.g2s = [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [S])[0]]
        self._lsrs, self._polys, self._host = {}, {}, {}

    def lsrs(self, n):
        """The Lagrange SRS of size n on the device: the inverse G1 NTT of the first n SRS points."""
        if n not in self._lsrs:
            out = self.torch.empty(8 * n, dtype=self.torch.int64, device="cuda")
            self.torch.cuda.synchronize()
            self.ctx.ntt_g1_dev(F.root_of_unity(n), self.d_srs.data_ptr(), out.data_ptr(), n, inverse=True)
            self.torch.cuda.synchronize()
            self._lsrs[n] = out
        return self._lsrs[n]

    def host_points(self, t, n):
        key = (t.data_ptr(), n)
        if key not in self._host:
            v = F.limbs_to_ints(t[:8 * n].cpu().numpy().view(np.uint64))
            self._host[key] = [(v[2 * i], v[2 * i + 1]) for i in range(n)]
        return self._host[key]

    def polys(self, n, batch, pitch, seed, special=False):
        """(coefficient limbs, evaluation limbs, [coefficient lists], [evaluation lists]): batch
        random polynomials of n coefficients at pitch `pitch`, the gaps filled with random values
        too; with `special` the last two are the zero polynomial and a constant."""
        key = (n, batch, pitch, seed, special)
        if key not in self._polys:
            omega = F.root_of_unity(n)
            a = F.random_limbs(batch * pitch, seed)
            e = F.random_limbs(batch * pitch, seed + 1)
            ints = F.limbs_to_ints(a)
            coefs = [ints[b * pitch:b * pitch + n] for b in range(batch)]
            if special and batch >= 3:
                coefs[-2] = [0] * n
                coefs[-1] = [ints[0]] + [0] * (n - 1)
            evals = [F.ntt(c, omega) for c in coefs]
            for b in range(batch):
                a[4 * b * pitch:4 * (b * pitch + n)] = F.ints_to_limbs(coefs[b])
                e[4 * b * pitch:4 * (b * pitch + n)] = F.ints_to_limbs(evals[b])
            self._polys[key] = (a, e, coefs, evals)
        return self._polys[key]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def world(ctx):
    return World(ctx)


def expect_open(coefs, z, weights):
    ys = [F.poly_eval(p, z) for p in coefs]
    num = sum(w * (F.poly_eval(p, S) - y) for w, p, y in zip(weights, coefs, ys)) % R
    return ys, enc(F.g1_mul(F.G1_GEN, num * inv(S - z) % R))


def expect_commit(p):
    return enc(F.g1_mul(F.G1_GEN, F.poly_eval(p, S)))


def pick_z(kind, n, rng):
    omega = F.root_of_unity(n)
    if kind == "rand":
        return rng.randrange(R)
    if kind == "0":
        return 0
    if kind == "order2n":
        return F.root_of_unity(2 * n)  # z^n = -1: not in H
    k = {"1": 0, "w1": 1, "half": n // 2, "last": n - 1, "k2047": 2047, "k2048": 2048}[kind]
    return pow(omega, k % n, R)


def pick_weights(batch, rng, i):
    w = [rng.randrange(R) for _ in range(batch)]
    w[i % batch] = 0
    w[(i + 1) % batch] = 1
    return w


# ---------------------------------------------------------------- commit
@pytest.mark.parametrize("n", [1, 2, 8, 2048, 4096, 1 << 14])
@pytest.mark.parametrize("batch", [1, 3])
def test_commit_from_evaluations(ctx, world, n, batch):
    pitch = n + 3
    a, e, coefs, _ = world.polys(n, batch, pitch, 100 + n)
    da, de = world.dev(a), world.dev(e)
    from_evals = ctx.kzg_commit_dev(world.lsrs(n).data_ptr(), n, de.data_ptr(), n, pitch, batch)
    from_coefs = ctx.kzg_commit_dev(world.d_srs.data_ptr(), n, da.data_ptr(), n, pitch, batch)
    assert from_evals == from_coefs == [expect_commit(p) for p in coefs]


# ---------------------------------------------------------------- open
NS = [1, 2, 8, 64, 128, 256, 512, 2048, 4096, 1 << 14]
BATCHES = [1, 2, 7, 8, 9, 10, 11, 19, 20]
ZK = ["rand", "0", "1", "w1", "half", "last", "order2n"]
# every size with the batches and z cycling, every batch at n = 8, every z at n = 512 (two
# workgroups: partial sums in both cases of z) and at n = 4096 with the two chunk-boundary k
SHAPES = [(n, BATCHES[(2 * i + 1) % 9] if n <= 512 else [1, 2, 3][i % 3], ZK[i % 7]) for i, n in enumerate(NS)]
SHAPES += [(8, b, ZK[(i + 3) % 7]) for i, b in enumerate(BATCHES)]
SHAPES += [(512, 3, zk) for zk in ZK]
SHAPES += [(4096, 2, zk) for zk in ZK + ["k2047", "k2048"]]
SHAPES += [(2048, 1, "last"), (1 << 16, 1, "rand"), (1 << 16, 1, "half"), (1 << 17, 1, "rand"), (1 << 17, 1, "w1")]


@pytest.mark.parametrize("n,batch,zk", SHAPES, ids=[f"n{s[0]}-b{s[1]}-z{s[2]}" for s in SHAPES])
def test_open_dev_shapes(ctx, world, n, batch, zk):
    rng = random.Random(n * 131 + batch)
    a, e, coefs, _ = world.polys(n, batch, n, 7000 + n, special=True)
    z = pick_z(zk, n, rng)
    weights = pick_weights(batch, rng, n + batch)
    da, de = world.dev(a), world.dev(e)
    got = ctx.kzg_open_evals_dev(world.lsrs(n).data_ptr(), n, F.root_of_unity(n), de.data_ptr(), n, batch, z, weights)
    assert got == expect_open(coefs, z, weights)
    assert got == ctx.kzg_open_dev(world.d_srs.data_ptr(), n, da.data_ptr(), n, n, batch, z, weights)


def test_quotient_values_against_the_restated_formulas(ctx, world):
    """n = 8, batch = 3: W against msm_naive over the quotient's values from kzg_evals_expect,
    for z outside H and for every z in H."""
    n, omega = 8, F.root_of_unity(8)
    rng = random.Random(83)
    coefs = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    evals = [F.ntt(c, omega) for c in coefs]
    weights = [rng.randrange(R) for _ in range(3)]
    lsrs = world.host_points(world.lsrs(n), n)
    for z in [rng.randrange(R)] + [pow(omega, k, R) for k in range(n)]:
        ys, q = E.open_evals(evals, z, weights, n, omega)
        assert ctx.kzg_open_evals(lsrs, omega, evals, z, weights) == (ys, enc(F.msm_naive(lsrs, q))), z


def test_pitch_and_host_form(ctx, world):
    n, batch, pitch = 512, 9, 512 + 33
    a, e, coefs, evals = world.polys(n, batch, pitch, 8100)
    rng = random.Random(81)
    weights = [rng.randrange(R) for _ in range(batch)]
    omega = F.root_of_unity(n)
    lsrs = world.host_points(world.lsrs(n), n)
    de = world.dev(e)
    for z in (rng.randrange(R), pow(omega, 300, R)):
        want = expect_open(coefs, z, weights)
        assert ctx.kzg_open_evals_dev(world.lsrs(n).data_ptr(), n, omega, de.data_ptr(), pitch, batch, z, weights) == want
        assert ctx.kzg_open_evals(lsrs, omega, evals, z, weights) == want
        assert ctx.kzg_open_evals(lsrs, omega, evals, z, weights, pitch=pitch) == want


def test_constant_needs_no_srs(ctx, world):
    """n = 1: y_b = p_b[0] and W the identity whatever the SRS holds (here no point at all)."""
    import pbf

    d = world.dev(pbf.ints_to_limbs([5, 999, 6, 999]))
    junk = world.torch.full((8,), -1, dtype=world.torch.int64, device="cuda")
    assert ctx.kzg_open_evals_dev(junk.data_ptr(), 1, 1, d.data_ptr(), 2, 2, 12345, [3, 4]) == ([5, 6], (0, 0))
    assert ctx.kzg_open_evals([F.G1_GEN], 1, [[5], [6]], 1, [1, 1]) == ([5, 6], (0, 0))


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("count", [1, 4])
def test_fold_and_verify(ctx, world, count):
    import pbf

    n, batch = 64, 3
    omega = F.root_of_unity(n)
    rng = random.Random(95 + count)
    lsrs = world.host_points(world.lsrs(n), n)
    entries = []
    for i in range(count):
        coefs = [[rng.randrange(R) for _ in range(n)] for _ in range(batch)]
        evals = [F.ntt(c, omega) for c in coefs]
        z = pow(omega, rng.randrange(n), R) if i % 2 else rng.randrange(R)  # outside H, then inside
        weights = [rng.randrange(R) for _ in range(batch)]
        cs = ctx.kzg_commit(lsrs, evals)
        ys, w = ctx.kzg_open_evals(lsrs, omega, evals, z, weights)
        c, y = pbf.kzg_fold(cs, ys, weights, ctx)
        entries.append((c, z, y, w))
    rhos = [1] if count == 1 else [rng.randrange(1, R) for _ in range(count)]
    assert ctx.kzg_verify(world.g2s, entries, rhos) is True
    for pos in range(count):
        bad = list(entries)
        c, z, y, w = bad[pos]
        bad[pos] = (c, z, (y + 1) % R, w)
        assert ctx.kzg_verify(world.g2s, bad, rhos) is False, pos


# ---------------------------------------------------------------- _dev forms
def test_dev_forms_on_a_side_stream(ctx, world):
    torch = world.torch
    n, batch = 4096, 3
    a, e, coefs, evals = world.polys(n, batch, n, 9200)
    omega = F.root_of_unity(n)
    rng = random.Random(92)
    weights = [rng.randrange(R) for _ in range(batch)]
    z1, z2 = rng.randrange(R), pow(omega, 2048, R)
    lsrs = world.host_points(world.lsrs(n), n)
    host1 = ctx.kzg_open_evals(lsrs, omega, evals, z1, weights)
    host2 = ctx.kzg_open_evals(lsrs, omega, evals, z2, weights)
    d_l = world.lsrs(n)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        de = world.dev(e)
        # two openings back to back, nothing in between on the host
        dev1 = ctx.kzg_open_evals_dev(d_l.data_ptr(), n, omega, de.data_ptr(), n, batch, z1, weights,
                                      stream=st.cuda_stream)
        dev2 = ctx.kzg_open_evals_dev(d_l.data_ptr(), n, omega, de.data_ptr(), n, batch, z2, weights,
                                      stream=st.cuda_stream)
        # open, commit against the other basis (the window table is rebuilt), open again
        da = world.dev(a)
        com = ctx.kzg_commit_dev(world.d_srs.data_ptr(), n, da.data_ptr(), n, n, batch, stream=st.cuda_stream)
        dev3 = ctx.kzg_open_evals_dev(d_l.data_ptr(), n, omega, de.data_ptr(), n, batch, z1, weights,
                                      stream=st.cuda_stream)
        # the G1 NTT on the same stream: the Lagrange SRS again
        again = torch.empty_like(d_l)
        ctx.ntt_g1_dev(omega, world.d_srs.data_ptr(), again.data_ptr(), n, inverse=True, stream=st.cuda_stream)
    st.synchronize()
    assert dev1 == host1 == expect_open(coefs, z1, weights)
    assert dev2 == host2 == expect_open(coefs, z2, weights)
    assert dev3 == host1
    assert com == [expect_commit(p) for p in coefs]
    assert torch.equal(again, d_l)


# ---------------------------------------------------------------- errors
def test_argument_errors_return_einval_and_leave_the_context_usable(ctx, world):
    import pbf

    lib, h = ctx.lib, ctx.h
    n = 8
    omega = F.root_of_unity(n)
    u64 = lambda k: np.zeros(k, dtype=np.uint64)  # noqa: E731
    ptr = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
    lsrs = pbf._g1_limbs(world.host_points(world.lsrs(n), n))
    evals, out, one = u64(4 * 32), u64(8 * 4), pbf.ints_to_limbs([1])
    w2, wbad, big = pbf.ints_to_limbs([1, 1]), pbf.ints_to_limbs([1, R]), pbf.ints_to_limbs([R])
    om = lambda v: ptr(pbf.ints_to_limbs([v]))  # noqa: E731
    opn = lambda *a: lib.pbf_kzg_open_evals_bn254(h, *a)  # noqa: E731
    good = (ptr(lsrs), n, om(omega), ptr(evals), n, 2, ptr(one), ptr(w2), ptr(out), ptr(out))

    def but(i, v):
        a = list(good)
        a[i] = v
        return opn(*a)

    bad = [lib.pbf_kzg_open_evals_bn254(None, *good)]
    bad += [but(i, None) for i in (0, 2, 3, 6, 7, 8, 9)]                 # NULL pointers
    bad += [but(1, v) for v in (0, 3, 6, 12)]                            # n = 0, not a power of two
    bad += [but(5, 0), but(5, (1 << 16) + 1), but(4, n - 1)]             # batch, pitch < n
    bad += [but(6, ptr(big)), but(7, ptr(wbad))]                         # z, a weight >= r
    bad += [but(2, om(v)) for v in (F.root_of_unity(n // 2), F.root_of_unity(2 * n), 0, R)]  # omega
    assert bad == [pbf.PBF_EINVAL] * len(bad), bad
    # the _dev form checks the same before touching the device pointers
    d = world.dev(evals)
    for args in ((n, omega, d.data_ptr(), n - 1, 2, 1, [1, 1]), (n, omega, d.data_ptr(), n, 2, R, [1, 1]),
                 (n, F.root_of_unity(2 * n), d.data_ptr(), n, 2, 1, [1, 1]), (6, omega, d.data_ptr(), n, 2, 1, [1, 1])):
        with pytest.raises(pbf.PbfError) as e:
            ctx.kzg_open_evals_dev(world.lsrs(n).data_ptr(), *args)
        assert e.value.code == pbf.PBF_EINVAL
    # and the next valid call is right
    rng = random.Random(98)
    coefs = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    evs = [F.ntt(c, omega) for c in coefs]
    z, weights = rng.randrange(R), [rng.randrange(R), rng.randrange(R)]
    assert ctx.kzg_open_evals(world.host_points(world.lsrs(n), n), omega, evs, z, weights) == expect_open(coefs, z, weights)
