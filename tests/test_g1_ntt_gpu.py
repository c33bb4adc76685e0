"""The NTT over BN254 G1 (csrc/g1_ntt.hip) and the Lagrange-basis SRS, bit-exact: canonical affine
output is unique, so every comparison is word for word.

Expected values: the definition (an O(n^2) sum with the oracle's g1_mul / g1_add) at n = 2, 4, 8;
above that linearity: the transform of [k_j]G is [NTT_Fr(k)_i]G, the right side from the
oracle's Fr transform and pbf_g1_bn254_mul_base_dev.

Boundaries of the implementation, each with a size below, at and above it:
  * 64 lanes per workgroup, one butterfly each (n/2 = 64 at n = 128; the inverse's store pass, one
    point per lane, at n = 64): n = 32, 64, 128, 256;
  * the load pass's 256 threads per workgroup: n = 128, 256, 512;
  * stages of half-width below 64 map lanes position-major, the others group-major (the first
    group-major stage exists from n = 128), and a wave shares one twiddle from 64 groups on:
    n = 64, 128, 256 and up;
  * one stage per launch throughout: no boundary;
  * table tiling, 2^g1ntt.tile_log products per launch: by default 2^14, met by the butterflies at
    n = 2^15 and by the inverse's scaling at n = 2^14 (n = 2^13 .. 2^16 below); with the option at
    its minimum, 64, every size from 64 on runs several launches per stage (n = 64 .. 512)."""
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
import kzg_evals_expect as E  # noqa: E402

pytestmark = pytest.mark.gpu
R, Q = F.R, F.Q
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R
SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 1 << 13, 1 << 14, 1 << 15, 1 << 16]
TILED = [32, 64, 128, 256, 512]  # with g1ntt.tile_log = 6


def enc(p):
    return (0, 0) if p is None else p


def dec(p):
    return None if p == (0, 0) else p


class Dev:
    """Device helpers: [k]G on the device, points to and from tensors."""

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

    def ntt(self, ctx, omega, d_in, n, inverse, in_place):
        out = d_in.clone() if in_place else self.torch.full((8 * n,), -1, dtype=self.torch.int64, device="cuda")
        self.torch.cuda.synchronize()
        ctx.ntt_g1_dev(omega, out.data_ptr() if in_place else d_in.data_ptr(), out.data_ptr(), n, inverse=inverse)
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


_CASES = {}


def linear_case(dev, n, seed=0):
    """(scalars k, [k_j]G, [NTT(k)_i]G, [INTT(k)_i]G) of one size, computed once."""
    if (n, seed) not in _CASES:
        rng = random.Random(1000 * n + seed)
        ks = [rng.randrange(R) for _ in range(n)]
        omega = F.root_of_unity(n)
        _CASES[(n, seed)] = (omega, dev.mul_base(ks), dev.mul_base(F.ntt(ks, omega)),
                             dev.mul_base(F.ntt(ks, omega, inverse=True)))
    return _CASES[(n, seed)]


def check_all_forms(dev, ctx, n, host=True):
    torch = dev.torch
    omega, d_in, want_f, want_i = linear_case(dev, n)
    for inverse, want in ((False, want_f), (True, want_i)):
        for in_place in (False, True):
            got = dev.ntt(ctx, omega, d_in, n, inverse, in_place)
            assert torch.equal(got, want), (n, inverse, in_place)
        if host:
            assert ctx.ntt_g1(omega, dev.points(d_in), inverse=inverse) == dev.points(want), (n, inverse)


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("inverse", [False, True])
def test_definition(ctx, n, inverse):
    rng = random.Random(77 + n)
    pts = [F.g1_mul(F.G1_GEN, rng.randrange(1, 1 << 12)) for _ in range(n)]  # cheap to make, random points
    omega = F.root_of_unity(n)
    w = pow(omega, R - 2, R) if inverse else omega
    c = pow(n, R - 2, R) if inverse else 1
    want = []
    for k in range(n):
        acc = None
        for j in range(n):
            acc = F.g1_add(acc, F.g1_mul(pts[j], c * pow(w, j * k, R) % R))
        want.append(enc(acc))
    assert ctx.ntt_g1(omega, pts, inverse=inverse) == want


def test_n1_is_the_copy(ctx, dev):
    p = F.g1_mul(F.G1_GEN, 12345)
    for inverse in (False, True):
        assert ctx.ntt_g1(1, [p], inverse=inverse) == [p]
        assert ctx.ntt_g1(1, [(0, 0)], inverse=inverse) == [(0, 0)]
    d = dev.mul_base([12345])
    for in_place in (False, True):
        assert dev.points(dev.ntt(ctx, 1, d, 1, False, in_place)) == [p]


@pytest.mark.parametrize("n", SIZES)
def test_linearity(ctx, dev, n):
    check_all_forms(dev, ctx, n)


@pytest.mark.parametrize("n", TILED)
def test_linearity_small_tiles(tiled_ctx, dev, n):
    """Several launches per stage over one window table (g1ntt.tile_log = 6: 64 products)."""
    check_all_forms(dev, tiled_ctx, n)


def exit_cases(n, rng):
    omega = F.root_of_unity(n)
    a = rng.randrange(1, R)
    winv = pow(omega, R - 2, R)
    return omega, {
        "all-equal": [a] * n,                                   # doublings, then cancellations, then identities
        "all-zero": [0] * n,                                    # identities only
        "only-j1": [0, a] + [0] * (n - 2),                      # products of the identity; out[k] = [omega^k a]G
        "alternating": [a if j % 2 == 0 else R - a for j in range(n)],
        "one-output": [a * pow(winv, j, R) % R for j in range(n)],  # the whole sum lands in out[1]
    }


@pytest.mark.parametrize("n", [8, 1024])
def test_group_law_exits_inside_butterflies(ctx, dev, n):
    omega, cases = exit_cases(n, random.Random(5 + n))
    for name, ks in cases.items():
        d_in = dev.mul_base(ks)
        for inverse in (False, True):
            want_k = F.ntt(ks, omega, inverse=inverse)
            got = dev.ntt(ctx, omega, d_in, n, inverse, False)
            assert dev.torch.equal(got, dev.mul_base(want_k)), (name, inverse)
        fwd = F.ntt(ks, omega)
        if name == "all-zero":
            assert set(fwd) == {0}
        if name == "one-output":
            assert fwd[1] != 0 and set(fwd[:1] + fwd[2:]) == {0}
        if name == "all-equal":
            assert fwd[0] != 0 and set(fwd[1:]) == {0}


@pytest.mark.parametrize("n", [8, 1024, 4096])
def test_round_trip_word_for_word(ctx, dev, n):
    rng = random.Random(900 + n)
    ks = [rng.randrange(R) for _ in range(n)]
    for j in (0, 3, n // 2, n - 1):
        ks[j] = 0  # identity entries
    omega = F.root_of_unity(n)
    x = dev.mul_base(ks)
    f = dev.ntt(ctx, omega, x, n, False, False)
    assert dev.torch.equal(dev.ntt(ctx, omega, f, n, True, False), x)
    assert dev.torch.equal(dev.ntt(ctx, omega, f, n, True, True), x)
    if n == 8:
        pts = dev.points(x)
        assert pts[0] == (0, 0)
        assert ctx.ntt_g1(omega, ctx.ntt_g1(omega, pts), inverse=True) == pts


@pytest.mark.parametrize("n", [1, 2, 8, 1024, 4096])
def test_lagrange_srs(ctx, dev, n):
    srs = ctx.srs_create(S, n)
    omega = F.root_of_unity(n)
    L = E.lagrange_at(S, n, omega)
    got = ctx.srs_lagrange(srs, n)
    assert got == dev.points(dev.mul_base(L))
    assert ctx.srs_lagrange(srs, n, omega=omega) == got
    if n == 8:
        assert got == [enc(F.g1_mul(F.G1_GEN, l)) for l in L]
        # the forward transform of the powers, too: (S^n - 1) / (S omega^i - 1)
        assert ctx.ntt_g1(omega, srs[:n]) == dev.points(dev.mul_base(E.forward_at(S, n, omega)))


def test_errors(ctx, dev):
    import pbf

    lib, h = ctx.lib, ctx.h
    n = 8
    omega = F.root_of_unity(n)
    pts = dev.points(dev.mul_base(list(range(1, n + 1))))
    a = pbf._g1_limbs(pts)
    out = np.zeros(8 * n, dtype=np.uint64)
    d_in = dev.mul_base(list(range(1, n + 1)))
    d_out = dev.torch.full((8 * n,), -1, dtype=dev.torch.int64, device="cuda")
    dev.torch.cuda.synchronize()
    p64 = lambda x: pbf._ptr(x)  # noqa: E731
    w = lambda v: p64(pbf.ints_to_limbs([v]))  # noqa: E731

    def host(om, arr, o, nn, inverse=0):
        return lib.pbf_ntt_g1_bn254(h, om, arr, o, nn, inverse)

    def devf(om, i, o, nn, inverse=0):
        return lib.pbf_ntt_g1_bn254_dev(h, om, ctypes.c_void_p(i), ctypes.c_void_p(o), nn, inverse, None)

    EINVAL = 1
    bad_omegas = [F.root_of_unity(n // 2), F.root_of_unity(2 * n), 0, R, R + omega]
    for nn in (0, 3, 6, 12):
        assert host(w(omega), p64(a), p64(out), nn) == EINVAL
        assert devf(w(omega), d_in.data_ptr(), d_out.data_ptr(), nn) == EINVAL
    for om in bad_omegas:
        assert host(w(om), p64(a), p64(out), n) == EINVAL, om
        assert devf(w(om), d_in.data_ptr(), d_out.data_ptr(), n) == EINVAL, om
    assert host(w(1), p64(a), p64(out), 2) == EINVAL  # order 1, not 2
    # NULL arguments
    assert lib.pbf_ntt_g1_bn254(None, w(omega), p64(a), p64(out), n, 0) == EINVAL
    assert host(None, p64(a), p64(out), n) == EINVAL
    assert host(w(omega), None, p64(out), n) == EINVAL
    assert host(w(omega), p64(a), None, n) == EINVAL
    assert lib.pbf_ntt_g1_bn254_dev(None, w(omega), ctypes.c_void_p(d_in.data_ptr()),
                                    ctypes.c_void_p(d_out.data_ptr()), n, 0, None) == EINVAL
    assert devf(None, d_in.data_ptr(), d_out.data_ptr(), n) == EINVAL
    assert lib.pbf_ntt_g1_bn254_dev(h, w(omega), None, ctypes.c_void_p(d_out.data_ptr()), n, 0, None) == EINVAL
    assert lib.pbf_ntt_g1_bn254_dev(h, w(omega), ctypes.c_void_p(d_in.data_ptr()), None, n, 0, None) == EINVAL
    # host form: a point off the curve, a coordinate >= q (x + q is on the curve mod q)
    off = list(pts)
    off[5] = (pts[5][0], (pts[5][1] + 1) % Q)
    assert host(w(omega), p64(pbf._g1_limbs(off)), p64(out), n) == EINVAL
    big = list(pts)
    big[2] = (pts[2][0] + Q, pts[2][1])
    assert big[2][0] < 1 << 256
    assert host(w(omega), p64(pbf._g1_limbs(big)), p64(out), n) == EINVAL
    # nothing was enqueued or written
    dev.torch.cuda.synchronize()
    assert not out.any() and bool((d_out == -1).all())
    # and the same arguments, valid, succeed
    assert host(w(omega), p64(a), p64(out), n) == 0
    assert out.any()
