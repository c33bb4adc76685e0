"""The expected public-input proofs (tests/plonk_pi_expect.py, tests/golden/plonk_pi_bn254.json) against
the unmodified oracle, on the CPU: the fixture regenerates, the oracle's verifier accepts each
proof in its q' form and rejects it under one changed public input, and the O(n) evaluation
checker, given the ORIGINAL q, returns the proof's 7 fields as they stand (r_z has no PI term)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import plonk_bn254 as P  # noqa: E402
import plonk_pi_expect as E  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_pi_bn254.json")))["cases"]
IDS = [f"n{c['n']}-npub{c['npub']}-{c['mode']}" for c in GOLD]
PAPER = [c for c in GOLD if c["mode"] == "paper"]


def test_fixture_covers_the_cases():
    assert [(c["n"], c["npub"], c["mode"]) for c in GOLD] == \
        [(n, k, m) for n, k in E.CASES for m in ("reference", "paper")]
    assert E.CASES == [(8, 1), (8, 2), (16, 5), (16, 16)]


def test_fixture_regenerates():
    import gen_plonk_pi_golden as G

    assert G.cases() == GOLD


@pytest.mark.parametrize("case", GOLD, ids=IDS)
def test_circuits_pass_both_forms_of_the_gate_check(case):
    """The real equation and the reference's pre-check with its q_l * b term
    (constraints.rs:198-230), both including -pub_i; row 0 is a classic public row whose a wire is
    tied to the multiplication gate of row 1."""
    c = E.case_inputs(case["n"], case["npub"], case["mode"])
    (ql, qr, qo, qm, qc), (a, b, w), pub = c["q"], c["abc"], c["pub"]
    for i in range(case["n"]):
        p = pub[i] if i < case["npub"] else 0
        assert (ql[i] * a[i] + qr[i] * b[i] + qo[i] * w[i] + qm[i] * a[i] * b[i] + qc[i] - p) % E.R == 0
        assert (ql[i] * a[i] + ql[i] * b[i] + qo[i] * w[i] + qm[i] * a[i] * b[i] + qc[i] - p) % E.R == 0
    assert ql[0] == 1 and a[0] == pub[0] and b[0] == w[0] == 0
    assert c["copies"][0][0] == (0, 2) and c["copies"][0][1] == (0, 1) and a[1] == a[0] and qm[1] == 1


@pytest.mark.parametrize("case", PAPER, ids=[i for i, c in zip(IDS, GOLD) if c["mode"] == "paper"])
def test_oracle_verifier_accepts_and_rejects_in_q_prime_form(case):
    """Paper mode (an honest reference-mode proof does not verify)."""
    n = case["n"]
    c = E.case_inputs(n, case["npub"], "paper")
    st = E.setup(n)
    pts = [tuple(p) if p else None for p in case["pts"]]
    assert E.verify(st, c["q"], c["copies"], c["pub"], pts, case["fields"], c["chal"], c["u"], mode="paper")
    bad = list(c["pub"])
    bad[-1] = (bad[-1] + 1) % E.R
    assert not E.verify(st, c["q"], c["copies"], bad, pts, case["fields"], c["chal"], c["u"], mode="paper")


@pytest.mark.parametrize("case", GOLD, ids=IDS)
def test_evaluations_on_the_original_q_are_the_proof_fields(case):
    c = E.case_inputs(case["n"], case["npub"], case["mode"])
    got = P.evaluations_at_z(case["n"], c["q"], c["copies"], c["abc"], c["chal"], c["rnd"], mode=case["mode"])
    assert got == case["fields"]


def test_transformation_is_a_bijection_on_r_z_and_w_z():
    case = PAPER[0]
    c = E.case_inputs(case["n"], case["npub"], "paper")
    st = E.setup(case["n"])
    pts = [tuple(p) if p else None for p in case["pts"]]
    po, fo = E.to_oracle(st, c["pub"], c["chal"], pts, case["fields"])
    assert [i for i in range(9) if po[i] != pts[i]] == [7] and [i for i in range(7) if fo[i] != case["fields"][i]] == [5]
    assert E.from_oracle(st, c["pub"], c["chal"], po, fo) == (pts, case["fields"])


def test_scale_statements_satisfy_the_circuit():
    n = 64
    q, copies, a, b = E.scale_circuit(n, 7)
    for npub in (0, 1, 5, 64):
        pub, (wa, wb, wc) = E.scale_statement(a, b, npub, 11 + npub, fixed=((0, E.R - 1), (2, 0)))
        assert len(pub) == npub and (npub < 1 or pub[0] == E.R - 1) and (npub < 3 or pub[2] == 0)
        for i in range(n):
            assert (wa[i] * wb[i] - wc[i] - (pub[i] if i < npub else 0)) % E.R == 0
        cols = (wa, wb, wc)
        for col in range(3):
            for i, (kind, idx) in enumerate(copies[col]):
                assert cols[kind][idx - 1] == cols[col][i]
