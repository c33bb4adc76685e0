"""Operands and plain-integer models for tests/test_pairing_device_gpu.py and
tests/test_pairing_device_inputs.py: the Fq2 / Fq6 / Fq12 tower of csrc/pairing.hip, function by
function.

The reference of every tower operation is oracle/bn254_pairing.py (f2_*, f6_*, f12_*, final_exp);
Frobenius maps are f12_pow(x, q) and f12_pow(x, q^2), never the device's constants; a sparse or
five-coefficient product is the dense oracle product of the operand with zeros filled in. The
functions that work on raw integers have their specification as the reference: l9_reduce is
x % q, wm_r3's four combinations are (S0 - S1), (S2 - S0 - S1), (10 S0 - 8 S1 - S2) and
(9 S2 - 8 S0 - 10 S1) mod q, fq_inv of a raw value am is am^-1 R^2 mod q (R = 2^256), Fq::mul of
raw a, b is a b R^-1 mod q.

Beside the references stand restatements of how the device computes (l9_reduce_model,
wm_r3_model, almost_inverse, w_mul_model, frob1_model). They serve two ends on the CPU
(tests/test_pairing_device_inputs.py): they show what the chosen cases enter (both branches of
l9_reduce's last subtraction, the shift widths and the range of k of the almost-inverse), and,
with one plausible mistake switched on (`wrong`), that at least one chosen case would notice it.

An Fq2 is a pair of integers, an Fq6 three Fq2, an Fq12 the oracle's tower ((a0, a1, a2),
(b0, b1, b2)); "flat" is the device's w-basis, a list g of six Fq2 with g[k] the coefficient of
w^k. Everything is built deterministically from fixed seeds.
"""
import functools
import os
import random
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import bn254_pairing as B  # noqa: E402
from field_device_inputs import interleave, u256, from_u256  # noqa: E402,F401

Q = B.Q
RM = 1 << 256                      # the Montgomery radix
RM_INV = pow(RM, -1, Q)
ALL_ONES = (1 << 256) - 1          # the harness's marker of a stored value not below q
EDGE = (0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2)
Z2 = B.F2_ZERO
MAX2 = (Q - 1, Q - 1)


# ---- flat <-> tower, wire packing -----------------------------------------------------------------
def from_w(g):
    """flat w-basis -> tower: c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)."""
    return ((g[0], g[2], g[4]), (g[1], g[3], g[5]))


def to_w(x):
    return [x[0][0], x[1][0], x[0][1], x[1][1], x[0][2], x[1][2]]


def ints(coeffs):
    """A sequence of Fq2 -> the tuple of their integers (re, im, re, im, ...)."""
    return tuple(v for c in coeffs for v in c)


def f2s(vals):
    """The inverse of ints()."""
    return [(vals[i], vals[i + 1]) for i in range(0, len(vals), 2)]


def f12_ints(x):
    return tuple(B.f12_flat(x))


def pack(rows):
    """Tuples of integers below 2^256 -> (n, 4 * len(tuple)) uint64."""
    flat = [v for r in rows for v in r]
    return u256(flat).reshape(len(rows), -1)


def unpack(arr, width):
    vals = from_u256(arr)
    return [tuple(vals[i:i + width]) for i in range(0, len(vals), width)]


def pack_l9(rows):
    """Tuples of integers below 2^288 -> (n, 5 * len(tuple)) uint64 (9 limbs of 32 bits, padded)."""
    buf = b"".join(int(v).to_bytes(40, "little") for r in rows for v in r)
    return np.frombuffer(buf, dtype="<u8").reshape(len(rows), -1).copy()


# ---- operands of the tower -------------------------------------------------------------------------
def _coeff(rng):
    return rng.choice(EDGE) if rng.random() < 0.4 else rng.randrange(Q)


def _f2(rng):
    return (_coeff(rng), _coeff(rng))


def _rand2(rng):
    return (rng.randrange(Q), rng.randrange(Q))


Elem = namedtuple("Elem", "kind g")  # g: n Fq2 (Fq12: flat; Fq6: c0, c1, c2)
ELEM_KINDS = ("zero", "one", "max", "unit", "single", "fq6", "fq2", "fq", "edge", "random")


@functools.lru_cache(maxsize=None)
def elems(n, seed, nrandom=16, nedge=6):
    """Elements with n Fq2 coefficients (6: a flat Fq12, 3: an Fq6): all coefficients 0; the one;
    all coefficients q - 1 (the maximum of every lazy sum); a single nonzero coefficient at each
    position, once as the unit w^k and once as a general Fq2; elements of the subfields; coefficients
    drawn from EDGE and random; random."""
    rng = random.Random(seed)
    out = [Elem("zero", [Z2] * n), Elem("one", [B.F2_ONE] + [Z2] * (n - 1)), Elem("max", [MAX2] * n)]
    for k in range(n):
        out.append(Elem("unit", [B.F2_ONE if i == k else Z2 for i in range(n)]))
        c = (rng.randrange(1, Q), rng.choice((Q - 1, rng.randrange(1, Q))))
        out.append(Elem("single", [c if i == k else Z2 for i in range(n)]))
    if n == 6:
        out.append(Elem("fq6", [_rand2(rng) if i % 2 == 0 else Z2 for i in range(6)]))
        out.append(Elem("fq6", [MAX2 if i % 2 == 0 else Z2 for i in range(6)]))
    out.append(Elem("fq2", [_rand2(rng)] + [Z2] * (n - 1)))
    out.append(Elem("fq2", [(0, Q - 1)] + [Z2] * (n - 1)))
    out.append(Elem("fq", [(rng.randrange(2, Q), 0)] + [Z2] * (n - 1)))
    out += [Elem("edge", [_f2(rng) for _ in range(n)]) for _ in range(nedge)]
    out += [Elem("random", [_rand2(rng) for _ in range(n)]) for _ in range(nrandom)]
    return out


Pair = namedtuple("Pair", "kind x y")
PAIR_KINDS = ("zero", "one", "max", "single", "fq6", "fq2", "edge", "random")
PAIR_MIN = {"zero": 2, "one": 2, "max": 1, "fq6": 2, "fq2": 2, "edge": 6, "random": 16}


@functools.lru_cache(maxsize=None)
def pairs(n, seed):
    """Operand pairs with n Fq2 coefficients each. "single": a single nonzero coefficient at
    position i times one at position j, for every (i, j): every wrap i + j >= n of the product,
    each alone."""
    rng = random.Random(seed)
    es = elems(n, seed + 1)
    by = {k: [e.g for e in es if e.kind == k] for k in ELEM_KINDS}
    rnd = by["random"]
    out = [Pair("zero", by["zero"][0], rnd[0]), Pair("zero", rnd[1], by["zero"][0]),
           Pair("zero", by["zero"][0], by["zero"][0]),
           Pair("one", by["one"][0], rnd[2]), Pair("one", rnd[3], by["one"][0]),
           Pair("one", by["one"][0], by["one"][0]),
           Pair("max", by["max"][0], by["max"][0]), Pair("max", by["max"][0], rnd[4]),
           Pair("max", rnd[5], by["max"][0])]
    for i in range(n):
        for j in range(n):
            a = by["unit"][i] if (i + j) % 3 == 0 else by["single"][i]
            out.append(Pair("single", a, by["single"][j]))
    if n == 6:
        out += [Pair("fq6", by["fq6"][0], by["fq6"][1]), Pair("fq6", by["fq6"][1], rnd[6]),
                Pair("fq6", rnd[7], by["fq6"][0])]
    out += [Pair("fq2", by["fq2"][0], rnd[8]), Pair("fq2", rnd[9], by["fq2"][1]),
            Pair("fq2", by["fq2"][0], by["fq2"][1]), Pair("fq2", by["fq"][0], rnd[10])]
    out += [Pair("edge", a, b) for a, b in zip(by["edge"], reversed(by["edge"]))]
    out += [Pair("edge", a, [_f2(rng) for _ in range(n)]) for a in by["edge"][:2]]
    out += [Pair("random", [_rand2(rng) for _ in range(n)], [_rand2(rng) for _ in range(n)]) for _ in range(16)]
    return out


def kinds(cases, names):
    got = {k: 0 for k in names}
    for c in cases:
        got[c.kind] += 1
    return got


def check_pair_counts(cases, n):
    got = kinds(cases, PAIR_KINDS)
    assert got["single"] == n * n, got
    assert all(got[k] >= v for k, v in PAIR_MIN.items() if not (k == "fq6" and n != 6)), got
    assert any(c.x == [MAX2] * n and c.y == [MAX2] * n for c in cases)
    return got


# Fq2 itself: every combination of the edge coefficients, and random
@functools.lru_cache(maxsize=None)
def f2_values():
    rng = random.Random(0x2F2)
    return [(a, b) for a in EDGE for b in EDGE] + [_rand2(rng) for _ in range(24)]


@functools.lru_cache(maxsize=None)
def f2_pairs():
    rng = random.Random(0x2F3)
    sp = [(0, 0), (1, 0), (0, 1), MAX2, (Q - 1, 0), (0, Q - 1), ((Q - 1) // 2, (Q + 1) // 2), (1, Q - 1)]
    out = [(a, b) for a in sp for b in sp]
    out += [(_f2(rng), _f2(rng)) for _ in range(40)]
    out += [(_rand2(rng), _rand2(rng)) for _ in range(32)]
    return interleave(out, 0x2F4)


@functools.lru_cache(maxsize=None)
def f2_scalar_pairs():
    rng = random.Random(0x2F5)
    out = [(a, s) for a in f2_values()[:25:3] + [MAX2] for s in EDGE]
    out += [(_rand2(rng), rng.randrange(Q)) for _ in range(24)]
    return interleave(out, 0x2F6)


# ---- the flat-basis product as the workgroup engine forms it ------------------------------------------
SHAPE_J = {"dense": (0, 1, 2, 3, 4, 5), "line": (0, 1, 3), "five": (0, 1, 2, 3, 4)}


def fill(y, shape):
    """The dense flat operand of a shape's coefficients y[0 .. NJ)."""
    g = [Z2] * 6
    for jj, j in enumerate(SHAPE_J[shape]):
        g[j] = y[jj]
    return g


def w_conj(g):
    return [B.f2_neg(c) if k & 1 else c for k, c in enumerate(g)]


def w_mul_ref(x, y, shape="dense", negy=False):
    """The oracle's dense product of x with y's shape filled with zeros (negy: with its conjugate)."""
    yt = from_w(fill(y, shape))
    return to_w(B.f12_mul(from_w(x), B.f12_conj(yt) if negy else yt))


def w_mul_model(x, y, shape="dense", negy=False, wrong=None):
    """wm_r1 .. wm_r3 restated: 6 NJ products x_i y_j, the lane taking xi x_i (the register's second
    half) where i + j >= 6, the product negated for odd j under NEGY, summed per output
    coefficient. wrong: "no_wrap" the wrapped terms taken from the first half of the register;
    "no_neg" odd coefficients not negated under NEGY."""
    xi_x = [B.f2_mul(B.XI, c) for c in x]
    out = [Z2] * 6
    for i in range(6):
        for jj, j in enumerate(SHAPE_J[shape]):
            xa = xi_x[i] if i + j >= 6 and wrong != "no_wrap" else x[i]
            p = B.f2_mul(xa, y[jj])
            if negy and (j & 1) and wrong != "no_neg":
                p = B.f2_neg(p)
            out[(i + j) % 6] = B.f2_add(out[(i + j) % 6], p)
    return out


def xi_half(g):
    return [B.f2_mul(B.XI, c) for c in g]


# ---- Frobenius ----------------------------------------------------------------------------------------
_FROB = {}


def frob(x, power):
    """x^(q^power) of a tower Fq12 by the oracle's f12_pow (memoised: ~0.05 s per q)."""
    key = (f12_ints(x), power)
    if key not in _FROB:
        _FROB[key] = B.f12_pow(x, Q ** power)
    return _FROB[key]


@functools.lru_cache(maxsize=None)
def _frob1_consts():
    return [B.f2_pow(B.XI, k * (Q - 1) // 6) for k in range(6)]


def frob1_model(g, wrong=None):
    """w_frob1 / f12_frob1 restated on a flat element: g_k -> conj(g_k) xi^(k (q - 1) / 6).
    wrong = "tower_index": the constant indexed by the coefficient's place in tower order
    (w^0 w^2 w^4 w^1 w^3 w^5) instead of by k."""
    c = _frob1_consts()
    tower_place = [0, 3, 1, 4, 2, 5]  # flat k -> index in tower order
    return [B.f2_mul(B.f2_conj(g[k]), c[tower_place[k] if wrong == "tower_index" else k]) for k in range(6)]


@functools.lru_cache(maxsize=None)
def unary12():
    """Flat Fq12 operands of the one-operand functions."""
    return list(elems(6, 0x12A, nrandom=16, nedge=4))


# ---- the cyclotomic subgroup -----------------------------------------------------------------------------
def easy_part(f):
    """f^((q^6 - 1)(q^2 + 1)): in the cyclotomic subgroup, where inversion is conjugation."""
    f1 = B.f12_mul(B.f12_conj(f), B.f12_inv(f))
    return B.f12_mul(frob(f1, 2), f1)


@functools.lru_cache(maxsize=None)
def cyclotomic_cases():
    """Tower Fq12 elements of the cyclotomic subgroup: the easy part of random values, their
    conjugates, and 1. f12_csqr is a squaring only there; it is not tested outside."""
    rng = random.Random(0xC7C)
    out = [B.F12_ONE]
    for _ in range(9):
        c = easy_part(from_w([_rand2(rng) for _ in range(6)]))
        out += [c, B.f12_conj(c)]
    return out


# ---- final exponentiation ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def final_exp_cases():
    """(name, tower Fq12, the oracle's final_exp): at most 16 values, none zero."""
    rng = random.Random(0xFE)
    unit = lambda k: from_w([B.F2_ONE if i == k else Z2 for i in range(6)])  # noqa: E731
    vals = [("one", B.F12_ONE),
            ("fq", from_w([(rng.randrange(2, Q), 0)] + [Z2] * 5)),
            ("fq2", from_w([_rand2(rng)] + [Z2] * 5)),
            ("fq6", from_w([_rand2(rng) if i % 2 == 0 else Z2 for i in range(6)])),
            ("w", unit(1)), ("w3", unit(3)), ("max", from_w([MAX2] * 6)),
            ("cyclotomic", cyclotomic_cases()[1])]
    vals += [("random", from_w([_rand2(rng) for _ in range(6)])) for _ in range(4)]
    vals.append(("miller", B.miller_loop(B.g1_mul(B.G1_GEN, 0x1234567), B.g2_mul(B.G2_GEN, 0x89ABCDE))))
    assert len(vals) <= 16
    return [(n, v, B.final_exp(v)) for n, v in vals]


# ---- Fq::mul on raw operands below 2q (wm_r1) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mul_raw_pairs():
    rng = random.Random(0x3A1)
    sp = (0, 1, Q - 1, Q, Q + 1, 2 * Q - 2)
    out = [(a, b) for a in sp for b in sp]
    out += [(rng.randrange(2 * Q), rng.randrange(2 * Q)) for _ in range(200)]
    out += [(rng.randrange(Q, 2 * Q), rng.randrange(Q, 2 * Q)) for _ in range(60)]
    return interleave(out, 0x3A2)


def mul_raw_ref(a, b):
    return a * b * RM_INV % Q


# ---- l9_reduce ----------------------------------------------------------------------------------------------------
L9_BOUND = 340 * Q
Q_TOP = 3486998266802970666.0  # the device's divisor: q / 2^192, rounded up


def l9_reduce_model(x, margin=1e-9):
    """l9_reduce restated with Python's doubles: (result, d, the value before the last subtraction
    as the device holds it). margin = 0.0 is the mistake "the margin removed"."""
    w = [(x >> (32 * i)) & 0xFFFFFFFF for i in range(9)]
    top = (float(w[8]) * 18446744073709551616.0 + float(w[7]) * 4294967296.0) + float(w[6])
    est = top * (1.0 / Q_TOP) - margin
    d = int(est) if est > 0.0 else 0
    y = (x - d * Q) % (1 << 288)
    lo = y & ALL_ONES  # the device drops limb 8
    return (lo - Q if Q <= lo < 2 * Q else lo), d, y


@functools.lru_cache(maxsize=None)
def l9_cases():
    rng = random.Random(0x19)
    out = set()
    for d in range(341):
        for e in (-2, -1, 0, 1, 2, Q // 2, Q - 2, Q - 1):
            out.add(d * Q + e)
        # around d q with the low 192 bits (which the estimate does not see) all zero / all one
        hi = (d * Q >> 192) << 192
        out.update((hi, hi - 1, hi + (1 << 192), hi + (1 << 192) - 1))
    out.update((162 * Q - 1, 340 * Q - 1))
    out = sorted(v for v in out if 0 <= v < L9_BOUND)
    out += [rng.randrange(L9_BOUND) for _ in range(1500)]
    out += [rng.randrange(1 << rng.randrange(1, 262)) for _ in range(500)]
    return interleave(out, 0x1A)


# ---- wm_r3 ----------------------------------------------------------------------------------------------------------------
S_MAX = 6 * (Q - 1)


def wm_r3_ref(s0, s1, s2):
    return ((s0 - s1) % Q, (s2 - s0 - s1) % Q, (10 * s0 - 8 * s1 - s2) % Q, (9 * s2 - 8 * s0 - 10 * s1) % Q)


def wm_r3_model(s0, s1, s2, off54=54):
    """The four waves' combinations in 288-bit arithmetic with the offsets 6q, 12q, 54q, 108q, then
    l9_reduce. off54 = 48 is the mistake "the 54q offset lowered to 48q"."""
    m = 1 << 288
    v = ((s0 + 6 * Q - s1) % m, (s2 + 12 * Q - s0 - s1) % m, (10 * s0 + off54 * Q - 8 * s1 - s2) % m,
         (9 * s2 + 108 * Q - 8 * (s0 + s1) - 2 * s1) % m)
    return tuple(l9_reduce_model(x)[0] for x in v)


def _six(rng):
    return sum(rng.randrange(Q) for _ in range(6))


@functools.lru_cache(maxsize=None)
def wm_r3_cases():
    """(S0, S1, S2), each a sum of six canonical values: every combination of 0, q - 1, 6 (q - 1)
    and a random sum, then random triples."""
    rng = random.Random(0x3E3)
    out = []
    for a in range(4):
        for b in range(4):
            for c in range(4):
                out.append(tuple((0, Q - 1, S_MAX, _six(rng))[i] for i in (a, b, c)))
    out += [(_six(rng), _six(rng), _six(rng)) for _ in range(32)]
    return out


# the operands that minimise and maximise each of the four combinations
WM_R3_EXTREMES = ((0, S_MAX, 0), (S_MAX, 0, 0), (S_MAX, S_MAX, 0), (0, 0, S_MAX), (0, S_MAX, S_MAX),
                  (S_MAX, 0, S_MAX))


# ---- fq_inv: Kaliski's almost-inverse ------------------------------------------------------------------------------------
def almost_inverse(am, wrong=None):
    """fq_inv restated on integers: (result, k, shifts), shifts a list of (site, t) with site one
    of "first", "u" (u > v: u >>= t, s <<= t), "v" (v >>= t, r <<= t). Every intermediate is
    asserted to fit 256 bits and r to be below 2q before reduce_once, as the code assumes.
    wrong = "shr_word": u256_shr does one 32-bit word move too few."""
    if am == 0:  # no inverse: the code returns 0 (callers never pass it)
        return 0, 0, []

    def shr(a, t):
        if wrong == "shr_word" and t >= 32:
            return a >> (t - 32)
        return a >> t

    def shl(a, t):
        a <<= t
        assert a < RM, "u256_shl loses bits"
        return a

    def ctz(a):
        return (a & -a).bit_length() - 1

    u, v, r, s = Q, am, 0, 1
    k = ctz(v)
    shifts = [("first", k)]
    v = shr(v, k)
    done = False
    for _ in range(1024):
        if u > v:
            t = ctz(u - v)
            u = shr(u - v, t)
            r += s
            s = shl(s, t)
            shifts.append(("u", t))
            k += t
        else:
            d = (v - u) % RM
            s += r
            if d == 0:
                r = shl(r, 1)
                k += 1
                done = True
                break
            t = ctz(d)
            v = shr(d, t)
            r = shl(r, t)
            shifts.append(("v", t))
            k += t
        assert r < RM and s < RM
    assert done or wrong, "no exit within the guard"
    if wrong is None:
        assert r < 2 * Q and 254 <= k <= 508
    r = r - Q if r >= Q else r
    x = (Q - r) % RM
    inv2k = pow(2, -(k & 511), Q) * pow(RM, 3, Q) % Q  # g_inv2k[k]: 2^-k R^3, plain
    return x * inv2k * RM_INV % Q, k, shifts


def fq_inv_ref(am):
    return pow(am, -1, Q) * RM * RM % Q


def _else_branch_case(T):
    """am whose second step is the v-branch with a difference of exactly T (or T + 1) trailing
    zeros: u1 = (q - am) / 2 odd and am - u1 = c 2^T, so am = q - 2 u1 with u1 = (q - c 2^T) / 3."""
    for c in (1, 2, 4, 5):
        n = Q - c * (1 << T)
        if n > 0 and n % 3 == 0 and (n // 3) % 2 == 1:
            return Q - 2 * (n // 3)
    raise AssertionError(T)


INV_SHIFT_I = (0, 1, 31, 32, 33, 63, 64, 65, 96, 128, 160, 192, 224, 253)


@functools.lru_cache(maxsize=None)
def fq_inv_cases():
    """Raw operands of fq_inv, none zero: small and large values, 2^i (the first shift strips i
    bits) and q - 2^i (the first difference has i trailing zeros: u >>= i, s <<= i) for every i
    in 0..253, values whose second step shifts v and r by T bits, and random ones."""
    rng = random.Random(0x1F7)
    out = [1, 2, 3, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, 1 << 253, (1 << 253) + 1]
    for i in range(254):
        out += [1 << i, Q - (1 << i)]
    out += [_else_branch_case(T) for T in (31, 32, 33, 63, 64, 65, 96, 128, 160, 192, 224, 250)]
    out += [rng.randrange(1, Q) for _ in range(64)]
    out += [rng.randrange(1, 1 << rng.randrange(1, 254)) for _ in range(32)]
    return interleave(sorted(set(out)), 0x1F8)
