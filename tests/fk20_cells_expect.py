"""Python restatements of what the cell proofs must compute (include/pbf.h "KZG cell proofs"), over
plain integers mod r with the trapdoor S in place of the SRS points: srs[j] stands for S^j, a point
[v]G for v, [s^l]G2 for S^l. Cell i < k = n / l is the coset {omega^(i + k t) : t < l}, on which
x^l = c_i = omega^(i l). tests/test_fk20_cells_expect.py checks the slab route against the quotient
by long division on the CPU; the GPU tests take their expected values from here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254 as F  # noqa: E402
import fk20_expect as K  # noqa: E402

R = F.R


def ntt(values, root, inverse=False):
    """F.ntt, with the transform of size 1 the value itself."""
    return list(values) if len(values) == 1 else F.ntt(list(values), root, inverse=inverse)


def cell_points(n, l, omega, i):
    """The l points of cell i, in the order of out_y."""
    k = n // l
    return [pow(omega, i + k * t, R) for t in range(l)]


def h_direct(p, n, l, S):
    """h_m = sum_{j=0}^{n-1-(m+1)l} p_(j+(m+1)l) S^j for m < k; h_(k-1) = 0."""
    p, k = K.padded(p, n), n // l
    return [sum(p[j + (m + 1) * l] * pow(S, j, R) for j in range(n - (m + 1) * l)) % R for m in range(k)]


def a_slab(n, l, r, S):
    """a_r[t] = S^(r + l (k-2-t)) for t <= k - 2 and 0 for k - 1 <= t < 2k."""
    k = n // l
    return [pow(S, r + l * (k - 2 - t), R) if t <= k - 2 else 0 for t in range(2 * k)]


def b_slab(p, n, l, r):
    """b_r[u] = p_(r + l u) for u < k and 0 for k <= u < 2k."""
    p, k = K.padded(p, n), n // l
    return [p[r + l * u] for u in range(k)] + [0] * k


def xext_scalars(n, l, S, omega2):
    """The scalars of pbf_kzg_cells_setup_bn254's 2n points, slab-major."""
    w = pow(omega2, l, R)
    return [v for r in range(l) for v in ntt(a_slab(n, l, r, S), w)]


def h_by_slabs(p, n, l, S, omega2):
    """h through the l transforms of size 2k, root w = omega2^l: chat_i = sum_r bhat_(r,i)
    xext_(r,i), c = INTT(chat), h = c[k-1 .. 2k-1)."""
    k, w = n // l, pow(omega2, l, R)
    xext = xext_scalars(n, l, S, omega2)
    chat = [0] * (2 * k)
    for r in range(l):
        bhat = ntt(b_slab(p, n, l, r), w)
        for i in range(2 * k):
            chat[i] = (chat[i] + bhat[i] * xext[r * 2 * k + i]) % R
    c = ntt(chat, w, inverse=True)
    assert c[2 * k - 1] == 0 and (k == 1 or c[2 * k - 2] == 0)  # nothing wraps
    return c[k - 1:2 * k - 1]


def proofs_by_slabs(p, n, l, S, omega2):
    """W_i = sum_m c_i^m h_m, i < k: the forward transform of size k, root omega^l, of h."""
    return ntt(h_by_slabs(p, n, l, S, omega2), pow(omega2, 2 * l, R))


def divide(p, l, c):
    """(q, rem) with p = q (x^l - c) + rem, deg rem < l, by long division."""
    rem = [v % R for v in p]
    q = [0] * max(len(rem) - l, 0)
    for j in reversed(range(l, len(rem))):
        q[j - l] = rem[j]
        rem[j - l] = (rem[j - l] + c * rem[j]) % R
        rem[j] = 0
    return q, (rem + [0] * l)[:l]


def proofs_by_division(p, n, l, S, omega):
    """W_i = q_i(S) for the quotient of p by x^l - c_i."""
    k = n // l
    return [F.poly_eval(divide(K.padded(p, n), l, pow(omega, i * l, R))[0] or [0], S) for i in range(k)]


def cell_values(p, n, l, omega):
    """ys[i][t] = p(omega^(i + k t)): the transform of size n, cell-major."""
    k = n // l
    y = ntt(K.padded(p, n), omega)
    return [[y[i + k * t] for t in range(l)] for i in range(k)]


def interpolant(ys, n, l, omega, i):
    """The l coefficients of I_i from the cell's values: I_(i,j) = omega^(-i j) INTT_{l, omega^k}(ys)[j]."""
    k = n // l
    v = ntt(ys, pow(omega, k, R), inverse=True)
    return [v[j] * pow(omega, (-i * j) % n, R) % R for j in range(l)]


def identity_holds(entries, rhos, n, l, S, omega):
    """The verifier's check in the exponent, e(A, [s^l]G2) e(-B, G2) == 1 as A S^l == B, for
    entries (C, idx, ys, W) given as scalars."""
    a = sum(rho * w for rho, (_, _, _, w) in zip(rhos, entries)) % R
    b = 0
    for rho, (c, idx, ys, w) in zip(rhos, entries):
        i_s = F.poly_eval(interpolant(ys, n, l, omega, idx), S)
        b = (b + rho * (c - i_s + pow(omega, idx * l, R) * w)) % R
    return a * pow(S, l, R) % R == b
