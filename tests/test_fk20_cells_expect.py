"""The cell proofs' indices, pinned on the CPU (no GPU, no library): tests/fk20_cells_expect.py
restates h, the slabs a_r and b_r, the slice k - 1 + m, the interpolant and the verifier's identity
in Python integers. Here, for n = 1 .. 32, every l | n and len in {1, n/2, n - 1, n}, the slab route
must equal q_i(S) for the quotient by long division, the interpolant from values must equal
p mod (x^l - c_i), the weighted identity must hold, and l = 1 must reproduce
fk20_expect.openings_by_convolution."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import fk20_cells_expect as C  # noqa: E402
import fk20_expect as K  # noqa: E402

R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R
NS = [1, 2, 4, 8, 16, 32]


def lens_of(n):
    return sorted({1, n // 2, n - 1, n} & set(range(1, n + 1)))


def ls_of(n):
    return [l for l in NS if l <= n]


CASES = [(n, l, ln) for n in NS for l in ls_of(n) for ln in lens_of(n)]


def setup(n, l, ln, salt):
    rng = random.Random(1000 * n + 37 * l + ln + salt)
    omega2 = F.root_of_unity(2 * n)
    return rng, [rng.randrange(R) for _ in range(ln)], omega2, omega2 * omega2 % R


@pytest.mark.parametrize("n,l,ln", CASES)
def test_slab_route_is_the_quotient_at_s(n, l, ln):
    _, p, omega2, omega = setup(n, l, ln, 1)
    k = n // l
    assert C.h_by_slabs(p, n, l, S, omega2) == C.h_direct(p, n, l, S)
    assert C.h_direct(p, n, l, S)[k - 1] == 0
    got = C.proofs_by_slabs(p, n, l, S, omega2)
    assert len(got) == k
    assert got == C.proofs_by_division(p, n, l, S, omega)
    assert got == C.proofs_by_slabs(p, n, l, S, R - omega2)  # the other root of the same omega
    for i in range(k):  # the division is exact
        c = pow(omega, i * l, R)
        q, rem = C.divide(K.padded(p, n), l, c)
        back = list(rem) + [0] * (n - l)
        for j, v in enumerate(q):
            back[j + l] = (back[j + l] + v) % R
            back[j] = (back[j] - c * v) % R
        assert back == K.padded(p, n)
    if ln <= l:
        assert got == [0] * k


@pytest.mark.parametrize("n,l,ln", CASES)
def test_interpolant_from_values_is_the_remainder(n, l, ln):
    _, p, _, omega = setup(n, l, ln, 2)
    ys = C.cell_values(p, n, l, omega)
    for i in range(n // l):
        assert ys[i] == [F.poly_eval(p, x) for x in C.cell_points(n, l, omega, i)]
        assert all(pow(x, l, R) == pow(omega, i * l, R) for x in C.cell_points(n, l, omega, i))
        assert C.interpolant(ys[i], n, l, omega, i) == C.divide(K.padded(p, n), l, pow(omega, i * l, R))[1]


@pytest.mark.parametrize("n,l,ln", CASES)
def test_weighted_identity(n, l, ln):
    rng, p, omega2, omega = setup(n, l, ln, 3)
    k = n // l
    ys, ws, commit = C.cell_values(p, n, l, omega), C.proofs_by_slabs(p, n, l, S, omega2), F.poly_eval(p, S)
    p2 = [rng.randrange(R) for _ in range(n)]  # a second polynomial in the same check
    ys2, ws2, commit2 = C.cell_values(p2, n, l, omega), C.proofs_by_slabs(p2, n, l, S, omega2), F.poly_eval(p2, S)
    entries = [(commit, i, ys[i], ws[i]) for i in range(k)] + [(commit2, k - 1, ys2[k - 1], ws2[k - 1])]
    entries.append(entries[0])  # a repeated cell
    rhos = [rng.randrange(1, R) for _ in entries]
    assert C.identity_holds(entries, rhos, n, l, S, omega)
    assert C.identity_holds(entries[:1], [1], n, l, S, omega)
    bad = list(entries)
    c0, i0, y0, w0 = bad[0]
    bad[0] = (c0, i0, [(y0[0] + 1) % R] + y0[1:], w0)
    assert not C.identity_holds(bad, rhos, n, l, S, omega)
    bad[0] = (c0, i0, y0, (w0 + 1) % R)
    assert not C.identity_holds(bad, rhos, n, l, S, omega)
    if k > 1:
        bad[0] = (c0, (i0 + 1) % k, y0, w0)
        assert not C.identity_holds(bad, rhos, n, l, S, omega) or ln == 1


@pytest.mark.parametrize("n", NS)
def test_l_one_is_fk20(n):
    for ln in lens_of(n):
        _, p, omega2, _ = setup(n, 1, ln, 4)
        assert C.proofs_by_slabs(p, n, 1, S, omega2) == K.openings_by_convolution(p, n, S, omega2)
        assert C.xext_scalars(n, 1, S, omega2) == K.xext_scalars(n, S, omega2)
        assert C.h_direct(p, n, 1, S) == K.h_direct(p, n, S)


def test_whole_domain_as_one_cell():
    for n in NS:
        omega2 = F.root_of_unity(2 * n)
        assert C.xext_scalars(n, n, S, omega2) == [0] * (2 * n)
        assert C.proofs_by_slabs(list(range(1, n + 1)), n, n, S, omega2) == [0]
