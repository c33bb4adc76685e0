"""A plain-integer restatement of the recovery from cells (include/pbf.h "Recovery from cells";
csrc/kzg_recover.hip): the route through the vanishing polynomial of the missing cells, over
oracle/bn254.py and the helpers of tests/fk20_cells_expect.py. Cell i < k = n / l is the l values on
{omega^(i + k t) : t < l}, on which x^l = c_i = omega^(i l). tests/test_recover_expect.py checks it
against the polynomials the cells were made from; the GPU tests take input cells from here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import fk20_cells_expect as C  # noqa: E402

R = F.R
SHIFT = 5  # the coset g H of the division; the results do not depend on it


def z_of(n, l, omega, missing, y):
    """Z at a point with x^l = y: the product over the missing cells of (y - c_i)."""
    z = 1
    for i in missing:
        z = z * (y - pow(omega, i * l, R)) % R
    return z


def interpolant(cells, cell_idx, n, l, omega, shift=SHIFT):
    """The n coefficients (zero from count*l on) of the polynomial of degree < count*l that takes
    cells[j][t] at omega^(cell_idx[j] + k t): E Z on H, its inverse transform, both on the coset
    shift * H, the pointwise quotient, back."""
    k = n // l
    slot = {i: j for j, i in enumerate(cell_idx)}
    assert len(slot) == len(cell_idx) and all(0 <= i < k for i in slot)
    missing = [i for i in range(k) if i not in slot]
    ez = [0] * n
    for i, j in slot.items():
        zi = z_of(n, l, omega, missing, pow(omega, i * l, R))
        for t in range(l):
            ez[i + k * t] = cells[j][t] * zi % R
    c = C.ntt(ez, omega, inverse=True)  # R Z exactly: its degree is below n
    on_coset = C.ntt([v * pow(shift, j, R) % R for j, v in enumerate(c)], omega)
    gl = pow(shift, l, R)
    zc = [z_of(n, l, omega, missing, gl * pow(omega, m * l, R) % R) for m in range(k)]
    assert all(zc)  # shift^n != 1: Z has no zero on the coset
    q = [v * pow(zc[j % k], R - 2, R) % R for j, v in enumerate(on_coset)]
    inv = pow(shift, R - 2, R)
    return [v * pow(inv, j, R) % R for j, v in enumerate(C.ntt(q, omega, inverse=True))]


def recover(cells, cell_idx, n, l, length, omega, shift=SHIFT):
    """(the first `length` coefficients, every cell of that polynomial, consistent) as
    pbf_kzg_recover_cells_bn254 returns them for one polynomial."""
    r = interpolant(cells, cell_idx, n, l, omega, shift)
    poly = r[:length]
    return poly, C.cell_values(poly, n, l, omega), int(not any(r[length:]))


def known_cells(p, n, l, omega, cell_idx):
    """The input of a recovery: the cells cell_idx of p, in that order."""
    ys = C.cell_values(p, n, l, omega)
    return [list(ys[i]) for i in cell_idx]
