"""The pairing's field tower on the device, function by function, against the integers.

tests/test_pairing_gpu.py reaches csrc/pairing.hip only through the C ABI: points in, random
discrete logs. The places where that file could be subtly wrong (a quotient estimate at a
multiple of q, a lazy sum at its bound, an inverse whose loop shifts by whole words, a zero, one
or maximal coefficient, a compensating pair of errors in two product shapes) are hit by such
inputs with probability about 2^-250. tests/native/pairing_device_check.hip (built by
__graft_entry__.build() into tests/native/libpairing_device_check.so, linked against libpbf.so)
includes csrc/pairing.hip unchanged and calls its device functions one at a time on the operands of
tests/pairing_device_inputs.py; every result is compared for exact equality with
oracle/bn254_pairing.py (Frobenius as f12_pow(x, q), sparse products as dense ones with zeros
filled in) or, for the functions on raw integers, with their specification (x % q and the like).
The case counts are asserted before the GPU is called; tests/test_pairing_device_inputs.py shows
on the CPU what the cases enter and that a wrong kernel would be seen. Lane ops run one thread per
element on a count that is no multiple of 64, in a fixed shuffled order, so that neighbouring
lanes hold cases of different kinds; workgroup ops run one 256-thread workgroup per element. A
stored value that is not below q comes back as all-ones, which every test checks for separately.

Functions and exits entered, by test:
  f2_mul, f2_sqr, f2_mul_xi, f2_neg,    every combination of 0, 1, q - 1, (q +- 1) / 2 as
  f2_conj, f2_muls, f2_inv               coefficients, and random: test_fq2
  Fq::mul on raw operands < 2q           {0, 1, q - 1, q, q + 1, 2q - 2}^2, random below 2q and
  (kara_raw / u256_add_raw in wm_r1)     in [q, 2q)^2; the result required canonical: test_fq_mul_raw
  l9_reduce                              d q + {-2 .. 2, q // 2, q - 2, q - 1} for every d < 340,
                                         low 192 bits all zero / all one around every d q,
                                         162 q - 1, 340 q - 1; the estimate exact and one below,
                                         the last subtraction taken and not: test_l9_reduce
  wm_r3, l9_add_kq, l9_shl, l9_sub       S_c in {0, q - 1, 6 (q - 1), random}^3: the minimum (0, 12,
                                         54, 108) and maximum of all four waves: test_wm_r3
  fq_inv, u256_shr, u256_shl, u256_ctz,  2^i and q - 2^i for every i < 254 and values whose second
  u256_subb, g_inv2k                     step shifts v and r by 32 .. 250 bits: shifts of whole
                                         words at all three sites, k = 254 .. 507, the u == v exit
                                         (every case); fq_inv(0) = 0 as the code states: test_fq_inv
  f6_mul, f6_mul_01, f6_inv              zero, one, maximal, single coefficients at every pair of
                                         positions, subfield elements, random: test_fq6
  f12_mul, f12_sqr, f12_mul_line,        the same over six positions (every wrap i + j >= 6 alone):
  f12_conj, f12_frob1, f12_frob2         test_fq12_products, test_fq12_maps
  f12_csqr                               the cyclotomic subgroup only: test_cyclotomic_square
  w_mul<W_DENSE / W_LINE / W_FIVE>       dst distinct, == x, == y, == x == y; the coefficients of y
  (wm_r1, wm_r2, wm_r3), w_fill_xi       beyond the shape's hold other values; all 12 slots, the xi
                                         half checked: test_w_mul
  w_mul_dual<false / true>,              the same and dA == xB and the round of powu (dA == xA ==
  w_mul_pair<W_DENSE, W_FIVE>            yA == yB, dB == xB); the two products of different kinds:
                                         test_w_mul_dual
  w_frob1, w_frob2, w_conj, w_one,       dst distinct and in place; fq6_inv_flat with live values
  fq6_inv_flat + w_fill_xi (FE_INVN)     in the odd slots: test_w_maps, test_w_invn
  final_exp_w (make_fe_prog),            1, elements of Fq, Fq2, Fq6, w, w^3, all q - 1, a
  f12_final_exp (make_fe_seq)            cyclotomic element, random, a Miller value; against the
                                         oracle and each other bit for bit: test_final_exp
  load_consts, make_consts,              every workgroup op; the unit's own host functions fill the
  ensure_inv2k                           harness's constants and g_inv2k
  g2_mul_kernel                          tests/test_pairing_gpu.py test_g2_mul_matches_oracle
Deliberately not reachable:
  fq_inv(0) beyond its stated return of 0 (f2_inv and f6_inv of 0 are outside the contract);
  f12_csqr outside the cyclotomic subgroup: there it is not a squaring, and the final
  exponentiation calls it only after the easy part;
  Miller additions with T = +-Q, which cannot occur for Q of order r (the step count is below r);
  G2 inputs off the curve or outside the order-r subgroup: the ABI checks only that coordinates
  are below q, it does NOT validate curve or subgroup membership, and no test here covers what
  the pairing returns for such points.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pairing_device_inputs as P  # noqa: E402
from pairing_device_inputs import ALL_ONES, Q, Z2  # noqa: E402

B = P.B
pytestmark = pytest.mark.gpu
LIB = os.path.join(HERE, "native", "libpairing_device_check.so")

# op codes of pairing_device_check.hip
(F2_MUL, F2_SQR, F2_MUL_XI, F2_INV, F2_NEG, F2_CONJ, F2_MULS, FQ_INV_RAW, FQ_MUL_RAW, L9_REDUCE, F6_MUL, F6_MUL_01,
 F6_INV, F12_MUL, F12_SQR, F12_MUL_LINE, F12_CONJ, F12_FROB1, F12_FROB2, F12_CSQR, F12_FINAL_EXP) = range(21)
(W_MUL_DENSE, W_MUL_LINE, W_MUL_FIVE, W_DUAL, W_DUAL_NEG, W_PAIR_DENSE_FIVE) = range(40, 46)
(W_FROB1, W_FROB2, W_CONJ, W_ONE, W_INVN, WM_R3, W_FINAL_EXP) = range(50, 57)
MAX_COUNT = 1 << 14


class Harness:
    def __init__(self):
        assert os.path.exists(LIB), "tests/native/libpairing_device_check.so missing: run __graft_entry__.build()"
        self.lib = ctypes.CDLL(LIB)
        vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
        self.lib.pdc_run.restype = ctypes.c_int
        self.lib.pdc_run.argtypes = [ctypes.c_int, u64, u64, vp, vp, vp, sz]
        self.lib.pdc_layout.restype = ctypes.c_int
        self.lib.pdc_layout.argtypes = [ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int)]

    def run(self, op, a, b=None, p0=0, l9=False):
        """a, b: lists of tuples of plain integers (one tuple per element; l9: 288-bit values);
        returns one tuple of 256-bit integers per element."""
        lay = (ctypes.c_int * 4)()
        assert self.lib.pdc_layout(op, p0, 0, lay) == 0, "unknown op %d or parameter %d" % (op, p0)
        aw, bw, ow, wg = lay
        count = len(a)
        assert 0 < count <= MAX_COUNT and (wg or count % 64 != 0)
        a = np.ascontiguousarray(P.pack_l9(a) if l9 else P.pack(a))
        assert a.size == count * aw, (a.size, count, aw)
        if bw:
            assert len(b) == count
            b = np.ascontiguousarray(P.pack(b))
            assert b.size == count * bw
        out = np.empty(count * ow, dtype=np.uint64)
        rc = self.lib.pdc_run(op, p0, 0, a.ctypes.data, b.ctypes.data if bw else None, out.ctypes.data, count)
        if rc != 0:  # a HIP error is sticky for the process: nothing more may run on the device
            pytest.exit("pdc_run(op %d, %d) returned HIP error %d" % (op, p0, rc), returncode=3)
        return P.unpack(out.reshape(count, ow), ow // 4)


@pytest.fixture(scope="module")
def pdc():
    return Harness()


def check(got, want, what):
    """No stored value is the harness's marker of a result not below q; then exact equality."""
    assert len(got) == len(want), what
    bad = [i for i, g in enumerate(got) if ALL_ONES in g]
    assert not bad, "%s: %d of %d results hold a value not below q, first at %d" % (what, len(bad), len(got), bad[0])
    assert all(v < Q for g in got for v in g), what
    bad = [i for i in range(len(got)) if tuple(got[i]) != tuple(want[i])]
    assert not bad, "%s: %d of %d differ, first at %d: got %s, expected %s" % (
        what, len(bad), len(got), bad[0], got[bad[0]], tuple(want[bad[0]]))


def check_regs(got, want_flat, what):
    """Workgroup outputs (12 slots): slots 0..5 the expected flat value, slots 6..11 xi times them."""
    assert all(len(g) == 24 for g in got), what
    check([g[:12] for g in got], [P.ints(w) for w in want_flat], what)
    check([g[12:] for g in got], [P.ints(P.xi_half(P.f2s(g[:12]))) for g in got], what + ", xi half")


# ---- Fq2 ----------------------------------------------------------------------------------------------
def test_fq2(pdc):
    pairs = P.f2_pairs()
    assert len(pairs) >= 128 and (P.MAX2, P.MAX2) in pairs and (Z2, Z2) in pairs
    check(pdc.run(F2_MUL, [a for a, _ in pairs], [b for _, b in pairs]), [B.f2_mul(a, b) for a, b in pairs], "f2_mul")
    vals = P.interleave(P.f2_values(), 0xF2)
    assert set(vals) >= {(a, b) for a in P.EDGE for b in P.EDGE}
    check(pdc.run(F2_SQR, vals), [B.f2_mul(a, a) for a in vals], "f2_sqr")
    check(pdc.run(F2_MUL_XI, vals), [B.f2_mul(B.XI, a) for a in vals], "f2_mul_xi")
    check(pdc.run(F2_NEG, vals), [B.f2_neg(a) for a in vals], "f2_neg")
    check(pdc.run(F2_CONJ, vals), [B.f2_conj(a) for a in vals], "f2_conj")
    inv = [a for a in vals if a != Z2]
    assert len(inv) % 64 != 0
    check(pdc.run(F2_INV, inv), [B.f2_inv(a) for a in inv], "f2_inv")
    sp = P.f2_scalar_pairs()
    check(pdc.run(F2_MULS, [a for a, _ in sp], [(s,) for _, s in sp]), [B.f2_muls(a, s) for a, s in sp], "f2_muls")


# ---- raw integers: Fq::mul below 2q, l9_reduce, wm_r3, fq_inv -------------------------------------------
def test_fq_mul_raw(pdc):
    """Fq::mul as wm_r1 calls it: operands up to 2q - 2 (kara_raw's unreduced sums), the result
    canonical."""
    pairs = P.mul_raw_pairs()
    assert (2 * Q - 2, 2 * Q - 2) in pairs and sum(a >= Q and b >= Q for a, b in pairs) >= 60
    got = pdc.run(FQ_MUL_RAW, [(a,) for a, _ in pairs], [(b,) for _, b in pairs])
    check(got, [(P.mul_raw_ref(a, b),) for a, b in pairs], "Fq::mul raw")


def test_l9_reduce(pdc):
    cases = P.l9_cases()
    assert len(cases) >= 5000 and max(cases) == 340 * Q - 1
    have = set(cases)
    assert all(d * Q in have and d * Q - 1 in have and d * Q + Q - 1 in have for d in range(1, 340))
    check(pdc.run(L9_REDUCE, [(x,) for x in cases], l9=True), [(x % Q,) for x in cases], "l9_reduce")


def test_wm_r3(pdc):
    cases = P.wm_r3_cases()
    assert all(e in cases for e in P.WM_R3_EXTREMES) and len(cases) >= 96
    got = pdc.run(WM_R3, cases, l9=True)
    want = []
    for c in cases:
        e = P.wm_r3_ref(*c)
        want.append((e[0], e[1]) * 6 + (e[2], e[3]) * 6)  # slot k: waves 0, 1; slot 6 + k: waves 2, 3
    check(got, want, "wm_r3")


def test_fq_inv(pdc):
    cases = P.fq_inv_cases()
    assert len(cases) >= 600 and all(1 << i in cases and Q - (1 << i) in cases for i in P.INV_SHIFT_I)
    cases = cases + [0]  # outside the contract: the code states that it returns 0
    assert len(cases) % 64 != 0
    got = pdc.run(FQ_INV_RAW, [(a,) for a in cases])
    check(got, [(P.fq_inv_ref(a) if a else 0,) for a in cases], "fq_inv")
    assert got[-1] == (0,)


# ---- the lane engine's Fq6 and Fq12 -------------------------------------------------------------------------
def test_fq6(pdc):
    cases = P.interleave(P.pairs(3, 0x300), 0x301)
    P.check_pair_counts(cases, 3)
    xs, ys = [P.ints(c.x) for c in cases], [P.ints(c.y) for c in cases]
    check(pdc.run(F6_MUL, xs, ys), [P.ints(B.f6_mul(tuple(c.x), tuple(c.y))) for c in cases], "f6_mul")
    check(pdc.run(F6_MUL_01, xs, [P.ints(c.y[:2]) for c in cases]),
          [P.ints(B.f6_mul(tuple(c.x), (c.y[0], c.y[1], Z2))) for c in cases], "f6_mul_01")
    es = [e.g for e in P.elems(3, 0x302) if e.kind != "zero"]
    assert len(es) >= 30 and len(es) % 64 != 0
    check(pdc.run(F6_INV, [P.ints(g) for g in es]), [P.ints(B.f6_inv(tuple(g))) for g in es], "f6_inv")


@pytest.fixture(scope="module")
def pairs12():
    cases = P.interleave(P.pairs(6, 0x600), 0x601)
    print("Fq12 pairs:", P.check_pair_counts(cases, 6))
    return cases


def test_fq12_products(pdc, pairs12):
    tw = lambda g: P.f12_ints(P.from_w(g))  # noqa: E731
    xs, ys = [tw(c.x) for c in pairs12], [tw(c.y) for c in pairs12]
    check(pdc.run(F12_MUL, xs, ys), [tw(P.w_mul_ref(c.x, c.y)) for c in pairs12], "f12_mul")
    both = [c.x for c in pairs12] + [c.y for c in pairs12 if c.kind in ("random", "edge")]
    assert len(both) % 64 != 0
    check(pdc.run(F12_SQR, [tw(g) for g in both]), [tw(P.w_mul_ref(g, g)) for g in both], "f12_sqr")
    # the line A0 + B0 w + B1 w^3 from y's first three coefficients
    check(pdc.run(F12_MUL_LINE, xs, [P.ints(c.y[:3]) for c in pairs12]),
          [tw(P.w_mul_ref(c.x, c.y, "line")) for c in pairs12], "f12_mul_line")


@pytest.fixture(scope="module")
def unary12():
    es = P.unary12()
    got = P.kinds(es, P.ELEM_KINDS)
    assert got["unit"] == 6 and got["single"] == 6 and got["random"] >= 16 and all(got[k] for k in P.ELEM_KINDS), got
    towers = [P.from_w(e.g) for e in es]
    return es, {1: [P.to_w(P.frob(x, 1)) for x in towers], 2: [P.to_w(P.frob(x, 2)) for x in towers]}


def test_fq12_maps(pdc, unary12):
    es, frob = unary12
    tw = lambda g: P.f12_ints(P.from_w(g))  # noqa: E731
    xs = [tw(e.g) for e in es]
    assert len(xs) % 64 != 0
    check(pdc.run(F12_CONJ, xs), [tw(P.w_conj(e.g)) for e in es], "f12_conj")
    check(pdc.run(F12_FROB1, xs), [tw(g) for g in frob[1]], "f12_frob1")
    check(pdc.run(F12_FROB2, xs), [tw(g) for g in frob[2]], "f12_frob2")


def test_cyclotomic_square(pdc):
    """f12_csqr (Granger-Scott) on elements of the cyclotomic subgroup: the oracle's easy part of
    random values, their conjugates, and 1. Outside the subgroup the function is not a squaring
    (its formulas use x^(q^4) x = x^(q^2)) and is not tested there."""
    cases = P.cyclotomic_cases()
    assert B.F12_ONE in cases and len(cases) >= 17 and len(cases) % 64 != 0
    check(pdc.run(F12_CSQR, [P.f12_ints(x) for x in cases]), [P.f12_ints(B.f12_sqr(x)) for x in cases], "f12_csqr")


# ---- the workgroup engine -----------------------------------------------------------------------------------------
W_SHAPES = {W_MUL_DENSE: "dense", W_MUL_LINE: "line", W_MUL_FIVE: "five"}


@pytest.mark.parametrize("alias", [0, 1, 2, 3], ids=["distinct", "dst_is_x", "dst_is_y", "dst_is_x_is_y"])
@pytest.mark.parametrize("op", list(W_SHAPES), ids=list(W_SHAPES.values()))
def test_w_mul(pdc, pairs12, op, alias):
    shape = W_SHAPES[op]
    got = pdc.run(op, [P.ints(c.x) + P.ints(c.y) for c in pairs12], p0=alias)
    want = [P.w_mul_ref(c.x, c.x if alias == 3 else c.y, shape) for c in pairs12]
    check_regs(got, want, "w_mul<%s>, alias %d" % (shape, alias))


DUAL_ALIAS = ["distinct", "dst_is_x", "dst_is_y", "squares", "dA_is_xB", "powu_round"]


@pytest.mark.parametrize("alias", range(6), ids=DUAL_ALIAS)
@pytest.mark.parametrize("op", [W_DUAL, W_DUAL_NEG, W_PAIR_DENSE_FIVE], ids=["dual", "dual_neg", "pair_dense_five"])
def test_w_mul_dual(pdc, pairs12, op, alias):
    """Two products in one set of rounds; product B's operands are product A's seven places on, so
    the two are of different kinds."""
    pa = pairs12
    pb = pairs12[7:] + pairs12[:7]
    assert sum(a.kind != b.kind for a, b in zip(pa, pb)) >= len(pa) // 2
    got = pdc.run(op, [P.ints(c.x) + P.ints(c.y) for c in pa], [P.ints(c.x) + P.ints(c.y) for c in pb], p0=alias)
    want_a, want_b = [], []
    for a, b in zip(pa, pb):
        ya = a.x if alias in (3, 5) else a.y
        yb = b.x if alias == 3 else (a.x if alias == 5 else b.y)
        want_a.append(P.w_mul_ref(a.x, ya))
        want_b.append(P.w_mul_ref(b.x, yb, "five" if op == W_PAIR_DENSE_FIVE else "dense", negy=op == W_DUAL_NEG))
    check_regs([g[:24] for g in got], want_a, "product A, alias %s" % DUAL_ALIAS[alias])
    check_regs([g[24:] for g in got], want_b, "product B, alias %s" % DUAL_ALIAS[alias])


@pytest.mark.parametrize("alias", [0, 1], ids=["distinct", "in_place"])
def test_w_maps(pdc, unary12, alias):
    es, frob = unary12
    xs = [P.ints(e.g) for e in es]
    check_regs(pdc.run(W_CONJ, xs, p0=alias), [P.w_conj(e.g) for e in es], "w_conj")
    check_regs(pdc.run(W_FROB1, xs, p0=alias), frob[1], "w_frob1")
    check_regs(pdc.run(W_FROB2, xs, p0=alias), frob[2], "w_frob2")
    if alias == 0:
        check_regs(pdc.run(W_ONE, xs), [[B.F2_ONE] + [Z2] * 5] * len(xs), "w_one")


def test_w_invn(pdc):
    """final_exp_w's FE_INVN step: fq6_inv_flat on slots 0, 2, 4 (the odd slots hold other values
    and come back zero), then w_fill_xi."""
    es = [e.g for e in P.elems(3, 0x302) if e.kind != "zero"]
    junk = P.unary12()[-1].g
    xs = [[g[0], junk[1], g[1], junk[3], g[2], junk[5]] for g in es]
    want = []
    for g in es:
        i = B.f6_inv(tuple(g))
        want.append([i[0], Z2, i[1], Z2, i[2], Z2])
    check_regs(pdc.run(W_INVN, [P.ints(x) for x in xs]), want, "fq6_inv_flat")


# ---- both final exponentiations -----------------------------------------------------------------------------------------
def test_final_exp(pdc):
    cases = P.final_exp_cases()
    assert 12 <= len(cases) <= 16
    want = [P.f12_ints(r) for _, _, r in cases]
    lane = pdc.run(F12_FINAL_EXP, [P.f12_ints(v) for _, v, _ in cases])
    check(lane, want, "f12_final_exp")
    wg = pdc.run(W_FINAL_EXP, [P.ints(P.to_w(v)) for _, v, _ in cases])
    check_regs(wg, [P.to_w(r) for _, _, r in cases], "final_exp_w")
    # the two engines, bit for bit
    assert [P.f12_ints(P.from_w(P.f2s(g[:12]))) for g in wg] == [tuple(g) for g in lane]
