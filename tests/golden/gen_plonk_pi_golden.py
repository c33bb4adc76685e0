#!/usr/bin/env python3
"""Golden proofs with public inputs (include/pbf.h "Public inputs") from the unmodified oracle, by the
derivation of tests/plonk_pi_expect.py: the oracle's proof on q' (q_c' = q_c - pub on the public
rows), with r_z and W_z moved by PI(z) and [v] commit((PI(x) - PI(z)) / (x - z)).
n = 8 (npub 1, 2) and n = 16 (npub 5, 16 = n), both modes. Every input of a case follows from its
(n, npub, mode) (plonk_pi_expect.case_inputs); the fixture holds those three, the 9 points and the
7 fields. Writes tests/golden/plonk_pi_bn254.json."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import plonk_pi_expect as E  # noqa: E402


def case(n, npub, mode, st=None):
    st = st or E.setup(n)
    c = E.case_inputs(n, npub, mode)
    pts, fs = E.prove(st, c["q"], c["copies"], c["abc"], c["pub"], c["chal"], c["rnd"], mode=mode)
    return {"n": n, "npub": npub, "mode": mode, "pts": [list(p) if p else None for p in pts], "fields": fs}


def cases():
    out = []
    for n, npub in E.CASES:
        st = E.setup(n)
        for mode in ("reference", "paper"):
            out.append(case(n, npub, mode, st))
    return out


if __name__ == "__main__":
    cs = cases()
    with open(os.path.join(HERE, "plonk_pi_bn254.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_plonk_pi_golden.py", "cases": cs}, f)
    print([(c["n"], c["npub"], c["mode"]) for c in cs])
