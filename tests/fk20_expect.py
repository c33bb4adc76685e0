"""Python restatements of what FK20 must compute (include/pbf.h "Every opening at once"), over
plain integers mod r with the trapdoor S in place of the SRS points: srs[k] stands for S^k, a point
[v]G for v. tests/test_fk20_expect.py checks the convolution route against the quotient from
oracle/bn254.py on the CPU; the GPU tests take their expected values from here."""
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


def inv_all(values):
    """[1 / v for v in values] with one inversion (no v is zero)."""
    pre = [1]
    for v in values:
        pre.append(pre[-1] * v % R)
    acc, out = inv(pre[-1]), [0] * len(values)
    for i in reversed(range(len(values))):
        out[i] = acc * pre[i] % R
        acc = acc * values[i] % R
    return out


def padded(p, n):
    """The n coefficients of p, those past len(p) zero."""
    assert 1 <= len(p) <= n
    return [c % R for c in p] + [0] * (n - len(p))


def h_direct(p, n, S):
    """h_m = sum_{k=0}^{n-2-m} p_(m+1+k) S^k for m < n; h_(n-1) = 0."""
    p = padded(p, n)
    return [sum(p[m + 1 + k] * pow(S, k, R) for k in range(n - 1 - m)) % R for m in range(n)]


def a_vector(n, S):
    """a_t = S^(n-2-t) for t <= n - 2 and 0 for n - 1 <= t < 2n."""
    return [pow(S, n - 2 - t, R) if t <= n - 2 else 0 for t in range(2 * n)]


def h_by_convolution(p, n, S, omega2):
    """h_m = c_(n-1+m) for c = a * b, taken as the cyclic convolution of size 2n through
    transforms with the root omega2 of order 2n: xext = NTT(a), bhat = NTT(b), c = INTT(xext bhat)."""
    if n == 1:
        return [0]
    xext = F.ntt(a_vector(n, S), omega2)
    bhat = F.ntt(padded(p, n) + [0] * n, omega2)
    c = F.ntt([x * y % R for x, y in zip(xext, bhat)], omega2, inverse=True)
    assert c[2 * n - 2] == 0 and c[2 * n - 1] == 0  # degree <= 2n - 3: nothing wraps
    return c[n - 1:2 * n - 1]


def xext_scalars(n, S, omega2):
    """The scalars of pbf_kzg_fk20_setup_bn254's 2n points."""
    return [0, 0] if n == 1 else F.ntt(a_vector(n, S), omega2)


def openings_by_convolution(p, n, S, omega2):
    """W_i = sum_m omega^(im) h_m, omega = omega2^2: the forward transform of size n of h."""
    h = h_by_convolution(p, n, S, omega2)
    return h if n == 1 else F.ntt(h, omega2 * omega2 % R)


def openings_trapdoor(p, n, S, omega):
    """W_i = (p(S) - p(omega^i)) / (S - omega^i); S outside <omega>."""
    ps = F.poly_eval(list(p), S)
    return [(ps - F.poly_eval(list(p), pow(omega, i, R))) * inv(S - pow(omega, i, R)) % R for i in range(n)]


def synthetic_quotient(p, z):
    """The coefficients of (p(x) - p(z)) / (x - z), by synthetic division (len(p) - 1 of them)."""
    q, acc = [], 0
    for c in reversed(list(p)):
        acc = (acc * z + c) % R
        q.append(acc)
    q.pop()  # the remainder p(z)
    return q[::-1]


def combine(polys, weights, n):
    """sum_b weights_b p_b as n coefficients."""
    full = [padded(p, n) for p in polys]
    return [sum(w * p[j] for w, p in zip(weights, full)) % R for j in range(n)]
