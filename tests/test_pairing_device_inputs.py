"""The case tables of tests/pairing_device_inputs.py, on the CPU: the counts that
tests/test_pairing_device_gpu.py relies on, the restatements of the device's methods against the
references, and, for each family, one plausible mistake switched on in the restatement: at least
one chosen case must then give a different result, or the cases could not notice a kernel with
that mistake."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pairing_device_inputs as P  # noqa: E402

B, Q = P.B, P.Q


def test_flat_and_tower_maps_round_trip():
    x = P.from_w(P.unary12()[-1].g)
    assert P.to_w(x) == P.unary12()[-1].g
    assert P.f2s(P.ints(P.to_w(x))) == P.to_w(x)
    # w * w = v: flat position 1 squared is flat position 2, the tower's c0.a1
    w = [B.F2_ONE if k == 1 else P.Z2 for k in range(6)]
    assert P.w_mul_ref(w, w) == [B.F2_ONE if k == 2 else P.Z2 for k in range(6)]
    assert P.from_w(P.w_mul_ref(w, w)) == ((P.Z2, B.F2_ONE, P.Z2), B.F6_ZERO)


def test_operand_counts():
    for n, seed in ((6, 0x600), (3, 0x300)):
        cases = P.pairs(n, seed)
        got = P.check_pair_counts(cases, n)
        assert got["random"] >= 16 and got["single"] == n * n
        # every wrap of the product alone: a single coefficient at i times one at j, all (i, j)
        pos = {(next(k for k in range(n) if c.x[k] != P.Z2), next(k for k in range(n) if c.y[k] != P.Z2))
               for c in cases if c.kind == "single"}
        assert pos == {(i, j) for i in range(n) for j in range(n)}
    es = P.unary12()
    got = P.kinds(es, P.ELEM_KINDS)
    assert got["unit"] == 6 and got["single"] == 6 and got["random"] >= 16 and got["fq6"] >= 1, got
    assert all(got[k] >= 1 for k in P.ELEM_KINDS), got
    coeffs = {v for e in es for c in e.g for v in c}
    coeffs |= {v for c in P.pairs(6, 0x600) for g in (c.x, c.y) for f in g for v in f}
    assert set(P.EDGE) <= coeffs
    assert len(P.f2_pairs()) % 64 and len(P.f2_scalar_pairs()) % 64 and len(P.mul_raw_pairs()) % 64
    sp = (0, 1, Q - 1, Q, Q + 1, 2 * Q - 2)
    assert {(a, b) for a in sp for b in sp} <= set(P.mul_raw_pairs())
    assert all(a < 2 * Q and b < 2 * Q for a, b in P.mul_raw_pairs())
    assert sum(a >= Q and b >= Q for a, b in P.mul_raw_pairs()) >= 60


def test_l9_reduce_cases_enter_both_branches_and_notice_a_missing_margin():
    cases = P.l9_cases()
    assert len(cases) % 64 != 0
    have = set(cases)
    for d in range(340):
        want = [d * Q + e for e in (-2, -1, 0, 1, 2, Q // 2, Q - 2, Q - 1)]
        assert all(v in have for v in want if 0 <= v < P.L9_BOUND), d
    assert {162 * Q - 1, 340 * Q - 1, 0} <= have and max(cases) == 340 * Q - 1
    low = (1 << 192) - 1
    assert sum(v & low == 0 for v in cases) >= 340 and sum(v & low == low for v in cases) >= 340
    exact = below = 0
    for x in cases:
        r, d, y = P.l9_reduce_model(x)
        assert r == x % Q and y < 2 * Q, hex(x)  # in [0, 2q) before the last subtraction
        assert d in (x // Q, x // Q - 1)
        exact += d == x // Q
        below += d == x // Q - 1
    print("l9_reduce: estimate exact %d, one below %d" % (exact, below))
    assert exact > 0 and below > 0
    # the last subtraction taken and not taken
    assert any(P.l9_reduce_model(x)[2] >= Q for x in cases) and any(P.l9_reduce_model(x)[2] < Q for x in cases)
    # mistake: the margin removed, d can be one too large
    assert any(P.l9_reduce_model(x, margin=0.0)[0] != x % Q for x in cases)


def test_wm_r3_cases_reach_the_bounds_and_notice_a_lower_offset():
    cases = P.wm_r3_cases()
    assert all(e in cases for e in P.WM_R3_EXTREMES)
    assert sum(all(v in (0, Q - 1, P.S_MAX) for v in c) for c in cases) >= 27
    assert sum(all(v not in (0, Q - 1, P.S_MAX) for v in c) for c in cases) >= 32
    assert all(0 <= v <= P.S_MAX for c in cases for v in c)
    # the two tight combinations come down to 54 and 108 at S = 6 (q - 1), not below
    assert 10 * 0 + 54 * Q - 8 * P.S_MAX - P.S_MAX == 54
    assert 9 * 0 + 108 * Q - 8 * P.S_MAX - 10 * P.S_MAX == 108
    for c in cases:
        assert P.wm_r3_model(*c) == P.wm_r3_ref(*c), c
    # mistake: the 54q offset lowered to 48q
    assert any(P.wm_r3_model(*c, off54=48) != P.wm_r3_ref(*c) for c in cases)


def test_product_cases_notice_a_wrong_wrap_and_a_missing_negation():
    cases = P.pairs(6, 0x600)
    for shape in P.SHAPE_J:
        for negy in (False, True):
            for c in cases:
                assert P.w_mul_model(c.x, c.y, shape, negy) == P.w_mul_ref(c.x, c.y, shape, negy), (shape, negy, c.kind)
    # mistake: the wrapped terms taken from the first half of the register. Every single-coefficient
    # pair with i + j >= 6 sees it, for every shape
    for shape, js in P.SHAPE_J.items():
        seen = [c for c in cases if P.w_mul_model(c.x, c.y, shape, wrong="no_wrap") != P.w_mul_ref(c.x, c.y, shape)]
        assert sum(c.kind == "single" for c in seen) >= 3 and any(c.kind == "max" for c in seen), shape
    # mistake: odd coefficients not negated under NEGB
    seen = [c for c in cases if P.w_mul_model(c.x, c.y, negy=True, wrong="no_neg") != P.w_mul_ref(c.x, c.y, negy=True)]
    assert sum(c.kind == "single" for c in seen) >= 18 and any(c.kind == "random" for c in seen)


def test_fq_inv_cases_span_the_loop_and_notice_a_dropped_word_shift():
    cases = P.fq_inv_cases()
    assert len(cases) % 64 != 0 and 0 not in cases and all(0 < a < Q for a in cases)
    have = set(cases)
    assert {1, 2, 3, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, 1 << 253, (1 << 253) + 1} <= have
    assert all(1 << i in have and Q - (1 << i) in have for i in P.INV_SHIFT_I)
    assert sum(1 << i in have and Q - (1 << i) in have for i in range(254)) == 254
    runs = {a: P.almost_inverse(a) for a in cases}  # asserts no 256-bit overflow and r < 2q inside
    for a, (r, k, _) in runs.items():
        assert r == P.fq_inv_ref(a), hex(a)
    ks = [k for _, k, _ in runs.values()]
    print("fq_inv: k from %d to %d" % (min(ks), max(ks)))
    assert min(ks) == 254 and max(ks) >= 500 and max(ks) <= 507
    assert runs[1 << 253][1] == 507
    for site in ("first", "u", "v"):
        ts = {t for _, _, sh in runs.values() for s, t in sh if s == site}
        assert all(any(lo <= t for t in ts) for lo in (32, 64, 128, 224)), (site, sorted(ts))
        assert any(32 <= t < 64 for t in ts) and any(64 <= t < 96 for t in ts) and any(t >= 224 for t in ts), site
    assert P.almost_inverse(0) == (0, 0, [])  # outside the contract: the code returns 0
    # mistake: a one-word shift dropped in u256_shr
    seen = 0
    for a in cases:
        try:
            seen += P.almost_inverse(a, wrong="shr_word")[0] != P.fq_inv_ref(a)
        except AssertionError:  # the wrong loop runs out of its bounds
            seen += 1
    assert seen >= 100


def test_frobenius_cases_notice_constants_in_tower_order():
    es = P.unary12()
    for e in es:
        assert P.frob1_model(e.g) == P.to_w(P.frob(P.from_w(e.g), 1)), e.kind
    # mistake: FROB1[k] indexed by tower order instead of flat order (right only for k = 0 and 5)
    seen = [e for e in es if P.frob1_model(e.g, wrong="tower_index") != P.to_w(P.frob(P.from_w(e.g), 1))]
    assert sum(e.kind == "unit" for e in seen) == 4 and any(e.kind == "random" for e in seen)
    # x^(q^2) twice is x^(q^4), and x^(q^6) is the conjugate: the references agree among themselves
    x = P.from_w(es[-1].g)
    assert P.frob(P.frob(P.frob(x, 2), 2), 2) == B.f12_conj(x)


def test_cyclotomic_and_final_exp_cases():
    cyc = P.cyclotomic_cases()
    assert B.F12_ONE in cyc and len(cyc) >= 17
    for c in cyc[:5]:
        # in the cyclotomic subgroup: x^(q^4) x = x^(q^2), and the conjugate is the inverse
        assert B.f12_mul(P.frob(P.frob(c, 2), 2), c) == P.frob(c, 2)
        assert B.f12_mul(c, B.f12_conj(c)) == B.F12_ONE
    fe = P.final_exp_cases()
    names = [n for n, _, _ in fe]
    assert len(fe) <= 16 and names.count("random") == 4
    assert set(names) == {"one", "fq", "fq2", "fq6", "w", "w3", "max", "cyclotomic", "random", "miller"}
    for n, v, want in fe:
        if n in ("one", "fq", "fq2", "fq6", "w", "w3"):  # (q^6 - 1)(q^2 + 1) kills Fq6 and w
            assert want == B.F12_ONE, n
        else:
            assert want != B.F12_ONE, n
