"""FK20's indices, pinned on the CPU (no GPU, no library): tests/fk20_expect.py restates h, the
vector a, the slice n - 1 + m and the trapdoor form in Python integers, and here the convolution
route must equal the quotient's value at S from the oracle's poly_eval and synthetic division,
for n = 1 .. 16 and len below and at n."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import fk20_expect as K  # noqa: E402

R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R
NS = [1, 2, 4, 8, 16]


def lens_of(n):
    return sorted({1, 2, n // 2 + 1, n - 1, n} & set(range(1, n + 1)))


CASES = [(n, ln) for n in NS for ln in lens_of(n)]


@pytest.mark.parametrize("n,ln", CASES)
def test_convolution_route_is_the_quotient_at_s(n, ln):
    rng = random.Random(31 * n + ln)
    p = [rng.randrange(R) for _ in range(ln)]
    omega2 = F.root_of_unity(2 * n)
    omega = omega2 * omega2 % R
    assert omega == F.root_of_unity(n) or n == 1
    got = K.openings_by_convolution(p, n, S, omega2)
    assert len(got) == n
    for i in range(n):
        z = pow(omega, i, R)
        q = K.synthetic_quotient(p, z)
        assert len(q) == ln - 1
        # the quotient is exact: q (x - z) + p(z) = p
        back = [0] * ln
        for j, c in enumerate(q):
            back[j + 1] = (back[j + 1] + c) % R
            back[j] = (back[j] - c * z) % R
        back[0] = (back[0] + F.poly_eval(p, z)) % R
        assert back == p
        assert got[i] == (F.poly_eval(q, S) if q else 0), (n, ln, i)
    assert got == K.openings_trapdoor(p, n, S, omega)


@pytest.mark.parametrize("n,ln", CASES)
def test_h_is_the_slice_of_the_convolution(n, ln):
    rng = random.Random(77 * n + ln)
    p = [rng.randrange(R) for _ in range(ln)]
    omega2 = F.root_of_unity(2 * n)
    h = K.h_direct(p, n, S)
    assert h[n - 1] == 0
    assert K.h_by_convolution(p, n, S, omega2) == h
    # the other root of the same omega gives the same h
    assert K.h_by_convolution(p, n, S, R - omega2) == h
    # against the plain product of a and b, index by index
    if n > 1:
        a, b = K.a_vector(n, S), K.padded(p, n)
        c = [sum(a[t] * b[k - t] for t in range(k + 1) if k - t < n) % R for k in range(2 * n)]
        assert c[n - 1:2 * n - 1] == h and c[2 * n - 2] == 0


def test_inv_all():
    vals = [3, R - 1, S, 1, 12345]
    assert K.inv_all(vals) == [K.inv(v) for v in vals]


def test_zero_and_constant_polynomials():
    for n in NS:
        omega2 = F.root_of_unity(2 * n)
        assert K.openings_by_convolution([0] * n, n, S, omega2) == [0] * n
        assert K.openings_by_convolution([12345], n, S, omega2) == [0] * n


def test_weighted_sum_opens_as_the_batch():
    """W of the batch is the opening of sum_b w_b p_b: the quotient is linear in p."""
    n, rng = 8, random.Random(5)
    omega2 = F.root_of_unity(2 * n)
    polys = [[rng.randrange(R) for _ in range(n - 1)] for _ in range(3)]
    weights = [rng.randrange(R), 0, 1]
    got = K.openings_by_convolution(K.combine(polys, weights, n), n, S, omega2)
    omega = omega2 * omega2 % R
    for i in range(n):
        z = pow(omega, i, R)
        num = sum(w * (F.poly_eval(p, S) - F.poly_eval(p, z)) for w, p in zip(weights, polys)) % R
        assert got[i] == num * K.inv(S - z) % R
