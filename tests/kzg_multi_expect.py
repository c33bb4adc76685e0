"""Python restatements of what the multi-point KZG opening must compute (include/pbf.h
"Multi-point KZG openings"; Boneh, Drake, Fisch, Gabizon 2020, section 4), over plain integers
mod r. tests/test_kzg_multi_expect.py checks them against schoolbook division and the real pairing
on the CPU; the GPU tests take their expected values from here.

Expected points use the trapdoor S of the test SRS, so each costs O(len) big-integer work and one
g1_mul:
    W  = [sum_b gamma^b (p_b(S) - r_b(S)) / Z_{S_b}(S)] G
    W' = [(sum_b gamma^b Z_{T \\ S_b}(z) (p_b(S) - r_b(z)) - Z_T(z) h(S)) / (S - z)] G
S must lie outside T and differ from z."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as F  # noqa: E402

R = F.R


def inv(a):
    a %= R
    assert a, "inverse of zero"
    return pow(a, R - 2, R)


def enc(p):
    return (0, 0) if p is None else p


def dec(p):
    return None if tuple(p) == (0, 0) else tuple(p)


def distinct(rng, k, avoid=()):
    """k distinct random field elements, none of them in `avoid`"""
    out = []
    while len(out) < k:
        v = rng.randrange(R)
        if v not in out and v not in avoid:
            out.append(v)
    return out


def members(mask, npts):
    return [j for j in range(npts) if (mask >> j) & 1]


def vanish(pts, js, x):
    """Z(x) = prod_{j in js} (x - t_j)"""
    r = 1
    for j in js:
        r = r * (x - pts[j]) % R
    return r


def interp_at(pts, js, ys, x):
    """r(x) for the interpolation r of (t_j, ys[j]), j in js, in product form: nothing is divided
    by x - t_j, so x may be one of the points."""
    total = 0
    for j in js:
        term = ys[j] % R
        for m in js:
            if m != j:
                term = term * (x - pts[m]) % R * inv(pts[j] - pts[m]) % R
        total = (total + term) % R
    return total


def poly_mul_linear(p, t):
    """p(x) (x - t)"""
    out = [0] * (len(p) + 1)
    for i, c in enumerate(p):
        out[i] = (out[i] - t * c) % R
        out[i + 1] = (out[i + 1] + c) % R
    return out


def long_division(c, d):
    """(quotient, remainder) of c by the monic d, schoolbook; the quotient padded to
    max(len(c) - 1, 0) coefficients as the library keeps it."""
    c, n, k = [x % R for x in c], len(c), len(d) - 1
    assert d[-1] == 1
    q = [0] * max(n - 1, 0)
    for i in range(n - 1, k - 1, -1):
        f = c[i]
        if f:
            q[i - k] = f
            for m in range(k + 1):
                c[i - k + m] = (c[i - k + m] - f * d[m]) % R
    return q, c[:k]


def synthetic_quotient(c, t):
    """The len(c) - 1 coefficients of quot(c, x - t): the recurrence of k_hs1..3."""
    q, s = [0] * (len(c) - 1), 0
    for j in range(len(c) - 1, 0, -1):
        s = (c[j] + t * s) % R
        q[j - 1] = s
    return q


def partial_fraction_quotient(c, pts, js):
    """quot(c, Z_S) = sum_{j in S} lambda_j quot(c, x - t_j), lambda_j = 1 / prod_{m != j} (t_j - t_m),
    on len(c) - 1 coefficients: what the division kernels compute."""
    out = [0] * (len(c) - 1)
    for j in js:
        lam = inv(vanish(pts, [m for m in js if m != j], pts[j]))
        for i, v in enumerate(synthetic_quotient(c, pts[j])):
            out[i] = (out[i] + lam * v) % R
    return out


def gamma_pows(gamma, batch):
    g = [1] * batch  # 0^0 = 1
    for b in range(1, batch):
        g[b] = g[b - 1] * gamma % R
    return g


def expect_ys(polys, pts, sets):
    """ys[b][j] = p_b(t_j) inside the set, 0 outside"""
    return [[F.poly_eval(p, t) if (mask >> j) & 1 else 0 for j, t in enumerate(pts)] for p, mask in zip(polys, sets)]


def h_at(vals, ys, pts, sets, gamma, S):
    """h(S) = sum_b gamma^b (p_b(S) - r_b(S)) / Z_{S_b}(S), vals[b] = p_b(S)"""
    npts, total = len(pts), 0
    for b, (v, g) in enumerate(zip(vals, gamma_pows(gamma, len(vals)))):
        js = members(sets[b], npts)
        total += g * (v - interp_at(pts, js, ys[b], S)) % R * inv(vanish(pts, js, S))
    return total % R


def w2_scalar(vals, ys, pts, sets, gamma, z, S):
    """the exponent of W': (sum_b gamma^b Z_{T \\ S_b}(z) (p_b(S) - r_b(z)) - Z_T(z) h(S)) / (S - z)"""
    npts, total = len(pts), 0
    for b, (v, g) in enumerate(zip(vals, gamma_pows(gamma, len(vals)))):
        js = members(sets[b], npts)
        rest = [j for j in range(npts) if j not in js]
        total += g * vanish(pts, rest, z) % R * (v - interp_at(pts, js, ys[b], z))
    total -= vanish(pts, range(npts), z) * h_at(vals, ys, pts, sets, gamma, S)
    return total % R * inv(S - z) % R


def expect_open(polys, pts, sets, gamma, S, vals=None):
    """(ys, W) of pbf_kzg_open_multi_bn254"""
    vals = vals or [F.poly_eval(p, S) for p in polys]
    ys = expect_ys(polys, pts, sets)
    return ys, enc(F.g1_mul(F.G1_GEN, h_at(vals, ys, pts, sets, gamma, S)))


def expect_finish(polys, pts, sets, gamma, z, S, vals=None, ys=None):
    """W' of pbf_kzg_open_multi_finish_bn254"""
    vals = vals or [F.poly_eval(p, S) for p in polys]
    ys = ys or expect_ys(polys, pts, sets)
    return enc(F.g1_mul(F.G1_GEN, w2_scalar(vals, ys, pts, sets, gamma, z, S)))


def verifier_sides(cvals, ys, pts, sets, gamma, z, w, w2):
    """The verifier's equation in the exponent, commitments and proofs given by their discrete
    logarithms (cvals[b], w, w2): (w2 S, F + z w2) with
    F = sum_b gamma^b Z_{T \\ S_b}(z) (C_b - r_b(z)) - Z_T(z) W; the opening is accepted iff
    lhs(S) == rhs, i.e. w2 * S == F + z * w2."""
    npts, f = len(pts), 0
    for b, (c, g) in enumerate(zip(cvals, gamma_pows(gamma, len(cvals)))):
        js = members(sets[b], npts)
        rest = [j for j in range(npts) if j not in js]
        f += g * vanish(pts, rest, z) % R * (c - interp_at(pts, js, ys[b], z))
    f -= vanish(pts, range(npts), z) * w
    return w2, (f + z * w2) % R


def accepts_in_exponent(cvals, ys, pts, sets, gamma, z, w, w2, S):
    lhs, rhs = verifier_sides(cvals, ys, pts, sets, gamma, z, w, w2)
    return lhs * S % R == rhs


def verifier_points(commits, ys, pts, sets, gamma, z, w, w2):
    """(W', F + z W') on the curve (points as (x, y) with (0, 0) the identity), for the pairing
    e(W', [s]G2) == e(F + z W', G2)"""
    npts, acc, gs = len(pts), None, 0
    for b, (c, g) in enumerate(zip(commits, gamma_pows(gamma, len(commits)))):
        js = members(sets[b], npts)
        rest = [j for j in range(npts) if j not in js]
        k = g * vanish(pts, rest, z) % R
        acc = F.g1_add(acc, F.g1_mul(dec(c), k))
        gs = (gs - k * interp_at(pts, js, ys[b], z)) % R
    acc = F.g1_add(acc, F.g1_mul(F.G1_GEN, gs))
    acc = F.g1_add(acc, F.g1_mul(dec(w), (-vanish(pts, range(npts), z)) % R))
    acc = F.g1_add(acc, F.g1_mul(dec(w2), z % R))
    return dec(w2), acc
