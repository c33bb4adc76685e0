"""The expectations of tests/kzg_evals_expect.py against oracle/bn254.py (ntt, poly_eval) on the CPU:
n = 1, 2, 8, 16, z outside H and every z = omega^k."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import kzg_evals_expect as E  # noqa: E402

R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R
NS = [1, 2, 8, 16]


def setup(n, seed):
    rng = random.Random(seed)
    omega = F.root_of_unity(n)
    p = [rng.randrange(R) for _ in range(n)]
    return rng, omega, p, F.ntt(p, omega)


def zs(n, omega, rng):
    return [rng.randrange(R), 0, F.root_of_unity(2 * n)] + [pow(omega, k, R) for k in range(n)]


@pytest.mark.parametrize("n", NS)
def test_lagrange_basis(n):
    """sum_i evals_i L_i(S) == p(S); L = the inverse transform of the powers of S; L_i(omega^j) = [i == j]."""
    rng, omega, p, ev = setup(n, 10 + n)
    L = E.lagrange_at(S, n, omega)
    assert sum(e * l for e, l in zip(ev, L)) % R == F.poly_eval(p, S)
    assert L == F.ntt([pow(S, j, R) for j in range(n)], omega, inverse=True)
    assert sum(L) % R == 1


@pytest.mark.parametrize("n", NS)
def test_forward_of_the_powers(n):
    omega = F.root_of_unity(n)
    assert E.forward_at(S, n, omega) == F.ntt([pow(S, j, R) for j in range(n)], omega)


@pytest.mark.parametrize("n", NS)
def test_barycentric_and_quotient(n):
    rng, omega, p, ev = setup(n, 20 + n)
    L = E.lagrange_at(S, n, omega)
    for z in zs(n, omega, rng):
        y = E.barycentric(ev, z, n, omega)
        assert y == F.poly_eval(p, z), (n, z)
        q = E.quotient_evals(ev, y, z, n, omega)
        assert sum(a * b for a, b in zip(q, L)) % R == (F.poly_eval(p, S) - y) * E.inv(S - z) % R, (n, z)
        # q is a polynomial of degree < n - 1: its top coefficient vanishes
        assert F.ntt(q, omega, inverse=True)[n - 1] == 0 or n == 1


@pytest.mark.parametrize("n", NS)
def test_batched_opening(n):
    rng, omega, _, _ = setup(n, 30 + n)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)] + [[0] * n, [7] + [0] * (n - 1)]
    evals = [F.ntt(p, omega) for p in polys]
    weights = [rng.randrange(R), 0, 1, rng.randrange(R), rng.randrange(R)]
    L = E.lagrange_at(S, n, omega)
    for z in zs(n, omega, rng):
        ys, q = E.open_evals(evals, z, weights, n, omega)
        assert ys == [F.poly_eval(p, z) for p in polys]
        num = sum(w * (F.poly_eval(p, S) - y) for w, p, y in zip(weights, polys, ys)) % R
        assert sum(a * b for a, b in zip(q, L)) % R == num * E.inv(S - z) % R
