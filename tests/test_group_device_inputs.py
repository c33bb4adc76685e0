"""CPU test of the operand sets of tests/test_group_device_gpu.py (tests/group_device_inputs.py).

The GPU test can only fail for a real error if its operands enter the exit that is wrong. These
tests run no GPU code: they check, with the Python restatements of the formulas, that
  - the restatements are the group law (against the oracle's g1_add / g1_mul on the discrete
    logs) on every chosen and random case, and the chain model and the masks predicted from the
    discrete logs agree;
  - the chosen operands contain every case the additions split into, random operands only the
    generic one;
  - a deliberately wrong model (the P = 0 test dropped; P + P told from P + (-P) by the
    operands' own Y, not cross-multiplied; is_identity reading X) disagrees with the group on the
    chosen operands and agrees with it on every random pair: random data cannot see it. The
    different-representation cases are the only ones that see the un-cross-multiplied comparison.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn254  # noqa: E402
import group_device_inputs as gdi  # noqa: E402
from group_device_inputs import Q, R  # noqa: E402

WRONG = ("no_p0", "y_plain", "id_x")


def _want(c):
    return gdi.log_sum([c.a, c.b])


def _misses(cases, fn, wrong):
    """The kinds of the cases on which fn's wrong model leaves the group."""
    return sorted({c.kind for c in cases if not gdi.group_ok(fn(c.p, c.q, wrong), _want(c))})


def test_points_are_the_oracles_multiples_and_lifts_are_representations():
    for a in gdi.LOGS:
        assert gdi.pt(a) == bn254.g1_mul(gdi.G, a) and bn254.g1_on_curve(gdi.pt(a))
    assert gdi.pt(1) == (1, 2) and gdi.pt(R - 1) == (1, Q - 2) and gdi.pt(0) is None
    # the points entered by additions (learn) are the multiples too
    for _, logs in gdi.chain_cases()[5][:2]:
        for t in logs:
            assert gdi.pt(t) == bn254.g1_mul(gdi.G, t)
    for c in gdi.pair_cases_chosen():
        for p, a in ((c.p, c.a), (c.q, c.b)):
            assert gdi.affine_of(p) == gdi.pt(a)
            assert max(p) < Q and pow(p[2], 3, Q) == p[3] * p[3] % Q
    # the sum by g1_add of the points is the sum of the logs
    for c in gdi.pair_cases_chosen()[:13]:
        assert _want(c) == bn254.g1_mul(gdi.G, (c.a + c.b) % R) if (c.a + c.b) % R else _want(c) is None


def test_models_are_the_group_law():
    for c in gdi.pair_cases_chosen() + gdi.pair_cases_random():
        assert gdi.group_ok(gdi.add(c.p, c.q), _want(c)), c.kind
    for c in gdi.mixed_cases_chosen() + gdi.mixed_cases_random():
        assert gdi.group_ok(gdi.madd(c.p, c.q), _want(c)), c.kind
    for p, a in gdi.unary_cases():
        assert gdi.group_ok(gdi.dbl(p), gdi.log_sum([a, a]))
        if a:
            assert gdi.group_ok(gdi.mdbl(gdi.pt(a)), gdi.log_sum([a, a]))
        assert gdi.to_affine_ref(p) == ((0, 0) if a == 0 else gdi.pt(a))
    p, a = next((p, a) for p, a in gdi.unary_cases() if a > 2 and p[2] != 1)
    for k in gdi.MUL_SMALL_KS:
        want = bn254.g1_mul(gdi.pt(a), k) if k else None
        assert gdi.group_ok(gdi.mul_small(p, k), want), k
        assert gdi.group_ok(gdi.mul_small(gdi.IDENTITY, k), None)


def test_exits_return_what_the_code_says():
    for c in gdi.pair_cases_chosen():
        r = gdi.add(c.p, c.q)
        if c.kind in ("p_id", "both_id"):
            assert r == c.q
        elif c.kind == "q_id":
            assert r == c.p
        elif c.kind.startswith("eq"):
            assert r == gdi.dbl(c.p)
        elif c.kind.startswith("neg"):
            assert r == gdi.IDENTITY
    for c in gdi.mixed_cases_chosen():
        r = gdi.madd(c.p, c.q)
        if c.kind == "p_id":
            assert r == (c.q[0], c.q[1], 1, 1)
        elif c.kind.startswith("eq"):
            assert r == gdi.mdbl(c.q)
        elif c.kind.startswith("neg"):
            assert r == gdi.IDENTITY


def test_operand_sets_contain_every_case():
    chosen = gdi.kinds(gdi.pair_cases_chosen(), gdi.PAIR_KINDS)
    assert all(chosen[k] >= 8 for k in gdi.PAIR_KINDS), chosen
    rand = gdi.kinds(gdi.pair_cases_random(), gdi.PAIR_KINDS)
    assert rand["generic"] == len(gdi.pair_cases_random()), rand
    mixed = gdi.kinds(gdi.mixed_cases_chosen(), gdi.MIXED_KINDS)
    assert all(mixed[k] >= 8 for k in gdi.MIXED_KINDS), mixed
    # the small and the large logs in every kind that has a point; both identity encodings
    for cases in (gdi.pair_cases_chosen(), gdi.mixed_cases_chosen()):
        for a in (1, R - 1):
            assert {c.kind for c in cases if a in (c.a, c.b)} >= {"generic", "eq_same", "eq_diff", "neg_same", "neg_diff", "p_id"}
        ids = [c.p for c in cases if c.kind == "p_id"]
        assert gdi.IDENTITY in ids and any(p[2] == 0 and p[0] > 1 for p in ids)
    # the shuffled arrays: no multiple of 64, every chosen case kept
    for arr, src in ((gdi.pair_cases(), gdi.pair_cases_chosen()), (gdi.mixed_cases(), gdi.mixed_cases_chosen())):
        assert len(arr) % 64 not in (0, 1) and set(src) <= set(arr)
    assert len(gdi.unary_cases()) % 64 not in (0, 1)


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_exit_is_seen_by_the_chosen_operands_only(wrong):
    seen_add = _misses(gdi.pair_cases_chosen(), gdi.add, wrong)
    seen_madd = _misses(gdi.mixed_cases_chosen(), gdi.madd, wrong)
    assert _misses(gdi.pair_cases_random(), gdi.add, wrong) == []
    assert _misses(gdi.mixed_cases_random(), gdi.madd, wrong) == []
    if wrong == "no_p0":  # ZZ3 = 0 comes out: right for P + (-P) by accident, wrong for P + P
        assert seen_add == ["eq_diff", "eq_same"] and seen_madd == ["eq_diff", "eq_same"]
    elif wrong == "y_plain":  # only two representations of one point tell the comparisons apart
        assert seen_add == ["eq_diff"] and seen_madd == ["eq_diff"]
    else:  # an identity with X != 0 enters the formulas; ZZ3 = 0 hides it when both are
        assert seen_add == ["p_id", "q_id"] and seen_madd == ["p_id"]


def test_chain_cases_and_masks():
    cases = gdi.chain_cases()
    assert set(cases) == {1, 2, 3, 5, gdi.MSM_CH}
    names = {n for k in cases for n, _ in cases[k]}
    assert names >= {"single", "P P", "P -P Q", "P P P", "P Q P+Q", "P Q -(P+Q)", "exceptional first",
                     "exceptional middle", "exceptional last", "43 copies", "43 distinct", "exceptional at 1",
                     "exceptional at 21", "exceptional at 42"}
    for k, items in cases.items():
        for name, logs in items:
            acc, dbl_mask, id_mask = gdi.chain([gdi.pt(t) for t in logs])
            assert (dbl_mask, id_mask) == gdi.chain_masks_from_logs(logs), name
            assert gdi.group_ok(acc, gdi.log_sum(logs)), name
            if name.startswith("exceptional at"):
                assert dbl_mask == 1 << int(name.split()[-1]) and id_mask == 0
            if name == "43 copies":
                assert dbl_mask == 2 and id_mask == 0
            if name == "43 distinct":
                assert dbl_mask == 0 and id_mask == 0 and len(set(logs)) == 43
            if name == "P Q P+Q":  # the exceptional return with a projective accumulator
                assert dbl_mask == 4 and id_mask == 0
            if name == "P -P Q":
                assert dbl_mask == 0 and id_mask == 2
