"""The restatement of the recovery from cells (tests/recover_expect.py) against the polynomials the
cells were made from, on the CPU: the route through the vanishing polynomial returns the original,
and for a changed value the interpolant of the given values with the stated flag."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import recover_expect as E  # noqa: E402
from recover_expect import C, F  # noqa: E402

R = F.R
CASES = [(64, 8, 32, 4), (64, 8, 29, 4), (64, 8, 33, 5), (16, 1, 8, 8), (16, 16, 16, 1), (64, 4, 64, 16), (32, 2, 3, 2),
         (8, 2, 1, 1)]


def setting(n, l, ln, count):
    rng = random.Random(1000 * n + 10 * l + ln)
    omega = F.root_of_unity(n) if n > 1 else 1
    p = [rng.randrange(R) for _ in range(ln)]
    idx = rng.sample(range(n // l), count)  # any order
    return rng, omega, p, idx, E.known_cells(p, n, l, omega, idx)


@pytest.mark.parametrize("n,l,ln,count", CASES)
def test_returns_the_original(n, l, ln, count):
    _, omega, p, idx, cells = setting(n, l, ln, count)
    assert E.interpolant(cells, idx, n, l, omega) == p + [0] * (n - ln)
    assert E.recover(cells, idx, n, l, ln, omega) == (p, C.cell_values(p, n, l, omega), 1)
    assert E.interpolant(cells, idx, n, l, omega, shift=7) == p + [0] * (n - ln)  # any shift


@pytest.mark.parametrize("n,l,ln,count", CASES)
def test_a_changed_value_gives_the_interpolant(n, l, ln, count):
    rng, omega, p, idx, cells = setting(n, l, ln, count)
    j, t = rng.randrange(count), rng.randrange(l)
    cells[j][t] = (cells[j][t] + 1 + rng.randrange(R - 1)) % R
    r = E.interpolant(cells, idx, n, l, omega)
    ys = C.cell_values(r, n, l, omega)
    assert [ys[i] for i in idx] == cells  # it takes the given values on the known cells
    assert not any(r[count * l:])  # and has degree below count * l
    assert any(r[ln:]) == (count * l > ln)
    poly, _, consistent = E.recover(cells, idx, n, l, ln, omega)
    assert poly == r[:ln] and consistent == int(count * l == ln)


def test_the_shift_has_no_power_of_two_order():
    """5^(2^28) != 1 in Fr: 5^n != 1 for every n <= 2^28, so Z has no zero on the coset 5 H."""
    assert pow(E.SHIFT, 1 << 28, R) != 1
