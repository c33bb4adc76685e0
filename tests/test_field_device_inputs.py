"""CPU test of the operand sets of tests/test_field_device_gpu.py (tests/field_device_inputs.py).

The GPU test can only fail for a real error if its operands enter the branch that is wrong.
These tests run no GPU code: they check, with the Python models of the case splits, that
  - the chosen operands reach every correction of the Goldilocks reduction, of add_mul_eps, of
    the Barrett product and of the 256-bit selects, while random operands alone do not;
  - a deliberately wrong model of one correction (the - EPS case of gl_red96 dropped; the
    256-bit add's select taken with > for >=) disagrees with the integer reference on the
    chosen operands, and agrees with it on every random operand: random data cannot see it;
  - the table MUL_POW2_REACH (which cases mul_pow2<S> can reach) is what the operand set gives.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_device_inputs as fdi  # noqa: E402
from field_device_inputs import FQ, FR, GOLD  # noqa: E402


def _mul_cases(pairs):
    return fdi.count_cases((fdi.red96_case(*fdi.mul_red96_args(a, b)) for a, b in pairs), fdi.RED96_CASES)


def test_edge_list_is_the_ntt_tests():
    import ast

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_ntt_gpu.py")
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.Assign) and len(n.targets) == 1
             and isinstance(n.targets[0], ast.Name) and n.targets[0].id == "EDGE_GL"]
    assert len(nodes) == 1
    expr = ast.fix_missing_locations(ast.Expression(nodes[0].value))
    assert eval(compile(expr, path, "eval"), {"__builtins__": {}, "GOLD": GOLD}) == fdi.EDGE_GL


def test_red96_model_is_the_reduction():
    for lo, hi in fdi.reduce128_pairs():
        assert fdi.red96_model(lo, hi & 0xFFFFFFFF, hi >> 32) == (lo + (hi << 64)) % GOLD


def test_mul_operands_reach_every_reduction_case():
    chosen = _mul_cases(fdi.gl_pairs_chosen())
    assert all(chosen[c] >= 3 for c in fdi.RED96_CASES), chosen
    rand = _mul_cases(fdi.gl_pairs_random())
    assert rand["c2"] == 0 and rand["both"] == 0 and rand["ge"] == 0, rand
    family = _mul_cases([(x << 48, y << 48) for x in (1, 2, 0x8000, 0xFFFF) for y in (1, 3, 0xFFFF)])
    assert family["c2"] == 12


def test_operands_reach_the_low_word_borrow_and_carry_of_the_correction():
    """c3 / c4 of gl_red96: the + EPS correction on a zero low word, the - EPS correction on an
    all-ones low word. Random operands reach neither."""
    mul = fdi.low_word_counts(fdi.mul_red96_args(a, b) for a, b in fdi.gl_pairs_chosen())
    red = fdi.low_word_counts((lo, hi & 0xFFFFFFFF, hi >> 32) for lo, hi in fdi.reduce128_pairs())
    xs = fdi.gl_unary()
    pw2 = fdi.low_word_counts(fdi.mul_pow2_red96_args(x, s) for s in range(33, 64) for x in xs)
    for got in (mul, red, pw2):
        assert got["c3"] >= 3 and got["c4"] >= 3, (mul, red, pw2)
    rand = fdi.low_word_counts(fdi.mul_red96_args(a, b) for a, b in fdi.gl_pairs_random())
    assert rand == {"c3": 0, "c4": 0}


def test_reduce128_and_add_mul_eps_operands_reach_every_case():
    r = fdi.count_cases((fdi.red96_case(lo, hi & 0xFFFFFFFF, hi >> 32) for lo, hi in fdi.reduce128_pairs()),
                        fdi.RED96_CASES)
    assert all(r[c] >= 3 for c in fdi.RED96_CASES), r
    a = fdi.count_cases((fdi.addmul_eps_case(lo, h) for lo, h in fdi.add_mul_eps_pairs()), fdi.ADDMUL_CASES)
    assert all(a[c] >= 3 for c in fdi.ADDMUL_CASES), a


def test_mul_pow2_reach_table():
    xs = fdi.gl_unary()
    for s in range(33, 64):
        got = fdi.count_cases((fdi.red96_case(*fdi.mul_pow2_red96_args(x, s)) for x in xs), fdi.RED96_CASES)
        assert tuple(c for c in fdi.RED96_CASES if got[c]) == fdi.MUL_POW2_REACH[s], (s, got)


def test_mul_pow2_cannot_reach_both():
    """The case "both" needs lo = 2^32 (1 + t), a multiple of 2^S, with t < h1 < 2^(S-32) (the derivation
    beside MUL_POW2_REACH). Every t is tried where that is few (S <= 44); for every S the least t
    that makes lo a multiple of 2^S, 2^(S-32) - 1, is already no smaller than the largest h1."""
    for s in range(33, 64):
        h1_max = (1 << (s - 32)) - 1
        if s <= 44:
            assert not any((((1 + t) << 32) % (1 << s)) == 0 for t in range(h1_max))
        t_min = (1 << (s - 32)) - 1
        assert ((1 + t_min) << 32) % (1 << s) == 0 and not t_min < h1_max
    # and the construction itself, on a shift small enough to try every operand of the form: S = 36,
    # hi = h0 + 2^32 h1 < 2^36 with h0 >= 2^32 - 16 (t < h1 < 16), any xl < 2^28 that is 0 or all ones
    s = 36
    for h1 in range(16):
        for h0 in range((1 << 32) - 16, 1 << 32):
            for xl in (0, 1, (1 << 28) - 1, (1 << 28) - 2):
                x = (((h1 << 32) | h0) << 28) | xl
                if x < GOLD:
                    assert fdi.red96_case(*fdi.mul_pow2_red96_args(x, s)) != "both"


def test_dropped_minus_eps_case_shows_on_chosen_operands_only():
    def wrong(pairs):
        bad = 0
        for a, b in pairs:
            bad += fdi.red96_model(*fdi.mul_red96_args(a, b), drop="c2") != a * b % GOLD
        return bad

    assert wrong(fdi.gl_pairs_chosen()) >= 3
    assert wrong(fdi.gl_pairs_random()) == 0
    # and the true model agrees everywhere
    for a, b in fdi.gl_pairs():
        assert fdi.red96_model(*fdi.mul_red96_args(a, b)) == a * b % GOLD


def test_wrong_256_bit_add_select_shows_on_chosen_operands_only():
    for p in (FR, FQ):
        chosen, rand = fdi.fp_pairs_chosen(p), fdi.fp_pairs_random(p)
        assert sum(fdi.fp_add_model(a, b, p, wrong=True) != (a + b) % p for a, b in chosen) >= 3
        assert all(fdi.fp_add_model(a, b, p, wrong=True) == (a + b) % p for a, b in rand)
        assert all(fdi.fp_add_model(a, b, p) == (a + b) % p for a, b in chosen + rand)


def test_256_bit_operands_take_both_sides_of_every_select():
    for p in (FR, FQ):
        pairs = fdi.fp_pairs(p)
        assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
        assert len(pairs) % 64 != 0
        for name, taken in (("add", [a + b >= p for a, b in pairs]), ("sub", [a < b for a, b in pairs]),
                            ("mul", [fdi.mont_unreduced(a, b, p) >= p for a, b in pairs]),
                            ("reduce_once", [x >= p for x in fdi.fp_reduce_inputs(p)])):
            assert min(sum(taken), len(taken) - sum(taken)) >= 16, name
        assert {a + b for a, b in pairs} >= {p - 1, p, p + 1}
        assert max(fdi.fp_reduce_inputs(p)) == 2 * p - 1


def test_mod32_operands_take_the_first_barrett_correction():
    for m in fdi.MOD32_MODULI:
        pairs = fdi.mod32_pairs(m)
        assert (m - 1, m - 1) in pairs and all(a < m and b < m for a, b in pairs)
        assert max(fdi.barrett_corrections(a, b, m) for a, b in pairs) <= 2  # "remainder < 3m"
    assert any(fdi.barrett_corrections(a, b, 3221225473) == 1 for a, b in fdi.mod32_pairs(3221225473))
    for m in ((1 << 32) - 5, (1 << 31) + 11):
        assert fdi.barrett_corrections(m - 1, m - 1, m) == 1


def test_lane_order_mixes_the_cases():
    """Neighbouring lanes differ: no wave of 64 consecutive products is in one case only, for
    the waves that hold chosen operands at all (the permutation is fixed, not a sort)."""
    pairs = fdi.gl_pairs()
    assert len(pairs) % 64 not in (0, 1)
    cases = [fdi.red96_case(*fdi.mul_red96_args(a, b)) for a, b in pairs]
    waves = [set(cases[i:i + 64]) for i in range(0, len(cases), 64)]
    assert sum(len(w) >= 2 for w in waves) == len(waves)
    assert sum(len(w) >= 3 for w in waves) >= len(waves) // 4
