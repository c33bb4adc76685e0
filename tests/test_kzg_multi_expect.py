"""tests/kzg_multi_expect.py, the integer model of the multi-point KZG opening, against schoolbook
long division, against itself in the exponent, and on the real pairing (CPU only)."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import kzg_multi_expect as X  # noqa: E402

R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R  # the trapdoor of the GPU tests


def rand_poly(rng, ln):
    return [rng.randrange(R) for _ in range(ln)]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_partial_fractions_equal_long_division(k):
    """quot(c, Z_S) from |S| synthetic divisions equals schoolbook division by Z_S for len = 1 .. 40,
    len <= |S| included (the quotient is zero there, and the sum gives canonical zeros)."""
    rng = random.Random(100 + k)
    for ln in range(1, 41):
        pts = X.distinct(rng, k, [S])
        if ln % 7 == 0:
            pts[0] = 0
        c = rand_poly(rng, ln)
        z = [1]
        for t in pts:
            z = X.poly_mul_linear(z, t)
        q, rem = X.long_division(c, z)
        assert X.partial_fraction_quotient(c, pts, list(range(k))) == q, (ln, k)
        if ln <= k:
            assert all(v == 0 for v in q)
        # and the remainder is the interpolation of c on S
        ys = [F.poly_eval(c, t) for t in pts]
        for x in pts + [rng.randrange(R)]:
            assert F.poly_eval(rem + [0], x) == X.interp_at(pts, list(range(k)), ys, x)


def h_coefficients(polys, pts, sets, gamma):
    """h as the library builds it: grouped by equal set, one partial-fraction quotient per group"""
    ln, npts = len(polys[0]), len(pts)
    g = X.gamma_pows(gamma, len(polys))
    h = [0] * (ln - 1)
    for mask in dict.fromkeys(sets):
        c = [sum(g[b] * p[i] for b, p in enumerate(polys) if sets[b] == mask) % R for i in range(ln)]
        for i, v in enumerate(X.partial_fraction_quotient(c, pts, X.members(mask, npts))):
            h[i] = (h[i] + v) % R
    return h


def cases():
    rng = random.Random(7)
    out = []
    for ln in range(1, 41):
        npts = 1 + (ln % 5)
        batch = 1 + rng.randrange(5)
        pts = X.distinct(rng, npts, [S])
        full = (1 << npts) - 1
        sets = [rng.randrange(1, full + 1) for _ in range(batch)]
        if batch > 2:
            sets[2] = sets[0]  # equal sets at non-adjacent indices
        gamma = (0, 1, rng.randrange(R))[ln % 3]
        z = (pts[0], 0, rng.randrange(R), rng.randrange(R))[ln % 4]
        out.append((ln, pts, sets, gamma, z, [rand_poly(rng, ln) for _ in range(batch)]))
    return out


def test_equation_holds_in_the_exponent():
    """W and W' of the model are the commitments of the polynomials the scheme names, and the
    verifier's equation holds for them for every len, with repeated sets, z in T, z = 0, gamma = 0
    and 1; a changed evaluation, gamma, z or mask breaks it."""
    for ln, pts, sets, gamma, z, polys in cases():
        ys = X.expect_ys(polys, pts, sets)
        vals = [F.poly_eval(p, S) for p in polys]
        w = X.h_at(vals, ys, pts, sets, gamma, S)
        h = h_coefficients(polys, pts, sets, gamma)
        assert (F.poly_eval(h, S) if h else 0) == w, ln
        # W' from coefficients: quot(sum_b gamma^b Z_{T \ S_b}(z) p_b - Z_T(z) h, x - z)
        npts, g = len(pts), X.gamma_pows(gamma, len(polys))
        f = [0] * ln
        for b, p in enumerate(polys):
            k = g[b] * X.vanish(pts, [j for j in range(npts) if not (sets[b] >> j) & 1], z) % R
            for i in range(ln):
                f[i] = (f[i] + k * p[i]) % R
        zt = X.vanish(pts, range(npts), z)
        for i, v in enumerate(h):
            f[i] = (f[i] - zt * v) % R
        q = X.synthetic_quotient(f, z)
        w2 = X.w2_scalar(vals, ys, pts, sets, gamma, z, S)
        assert (F.poly_eval(q, S) if q else 0) == w2, ln
        assert X.accepts_in_exponent(vals, ys, pts, sets, gamma, z, w, w2, S), ln
        if ln < 2 or z in pts:  # at z in T \ S_b the term of p_b vanishes: z is to be drawn after W
            continue
        bad = [list(r) for r in ys]
        j = X.members(sets[0], npts)[0]
        bad[0][j] = (bad[0][j] + 1) % R
        assert not X.accepts_in_exponent(vals, bad, pts, sets, gamma, z, w, w2, S), ln
        if npts > 1:  # with one point W' = W whatever z is
            assert not X.accepts_in_exponent(vals, ys, pts, sets, gamma, (z + 1) % R, w, w2, S), ln
        assert not X.accepts_in_exponent(vals, ys, pts, sets, gamma, z, w2, w, S) or w == w2, ln
        if len(polys) > 1:
            assert not X.accepts_in_exponent(vals, ys, pts, sets, (gamma + 1) % R, z, w, w2, S), ln


def test_tiny_case_on_the_real_pairing():
    """len = 5, batch = 3, npts = 3: e(W', [s]G2) == e(F + z W', G2) on oracle/bn254_pairing.py, and
    not with one evaluation changed."""
    rng = random.Random(11)
    pts = X.distinct(rng, 3, [S])
    sets = [0b111, 0b010, 0b101]
    polys = [rand_poly(rng, 5) for _ in range(3)]
    gamma, z = rng.randrange(R), rng.randrange(R)
    commits = [X.enc(F.g1_mul(F.G1_GEN, F.poly_eval(p, S))) for p in polys]
    ys, w = X.expect_open(polys, pts, sets, gamma, S)
    w2 = X.expect_finish(polys, pts, sets, gamma, z, S)
    s_g2 = B.g2_mul(B.G2_GEN, S)

    def check(ys_):
        lhs, rhs = X.verifier_points(commits, ys_, pts, sets, gamma, z, w, w2)
        return B.pairing_check([(lhs, s_g2), (B.g1_neg(rhs), B.G2_GEN)])

    assert check(ys)
    bad = [list(r) for r in ys]
    bad[2][2] = (bad[2][2] + 1) % R
    assert not check(bad)
