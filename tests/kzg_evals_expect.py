"""Python restatements of what KZG in evaluation form must compute (include/pbf.h "KZG in
evaluation form"), over plain integers mod r. tests/test_kzg_evals_expect.py checks them against
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


def lagrange_at(S, n, omega):
    """[L_i(S) for i < n], L_i(x) = (x^n - 1) omega^i / (n (x - omega^i)); S outside <omega>."""
    zh, ninv = (pow(S, n, R) - 1) % R, inv(n)
    out, w = [], 1
    for _ in range(n):
        out.append(zh * w % R * ninv % R * inv(S - w) % R)
        w = w * omega % R
    return out


def forward_at(S, n, omega):
    """The scalars of the forward G1 NTT of [S^j]G: sum_j (S omega^i)^j = (S^n - 1) / (S omega^i - 1)."""
    zh = (pow(S, n, R) - 1) % R
    return [zh * inv(S * pow(omega, i, R) - 1) % R for i in range(n)]


def in_domain(z, n, omega):
    """k with z = omega^k, or None."""
    if pow(z, n, R) != 1:
        return None
    w = 1
    for k in range(n):
        if w == z % R:
            return k
        w = w * omega % R
    raise AssertionError("omega does not generate the n-th roots of unity")


def barycentric(evals, z, n, omega):
    """p(z) from the n values p(omega^i)."""
    k = in_domain(z, n, omega)
    if k is not None:
        return evals[k] % R
    acc, w = 0, 1
    for i in range(n):
        acc = (acc + evals[i] * w % R * inv(w - z)) % R
        w = w * omega % R
    return (-(pow(z, n, R) - 1)) * inv(n) % R * acc % R


def quotient_evals(c, y_c, z, n, omega):
    """The values on <omega> of (c(x) - y_c) / (x - z), c given by its values and y_c = c(z)."""
    k = in_domain(z, n, omega)
    pw = [pow(omega, i, R) for i in range(n)]
    q = [0 if i == k else (c[i] - y_c) * inv(pw[i] - z) % R for i in range(n)]
    if k is not None:
        q[k] = (-inv(pw[k])) * sum(pw[i] * q[i] for i in range(n) if i != k) % R
    return q


def open_evals(evals, z, weights, n, omega):
    """([y_b], the quotient's values) of the batched opening of pbf_kzg_open_evals_bn254."""
    ys = [barycentric(e, z, n, omega) for e in evals]
    c = [sum(w * e[i] for w, e in zip(weights, evals)) % R for i in range(n)]
    y_c = sum(w * y for w, y in zip(weights, ys)) % R
    return ys, quotient_evals(c, y_c, z, n, omega)
