#!/usr/bin/env python3
"""The Fiat-Shamir challenges (include/pbf.h "Fiat-Shamir") of the committed golden proofs of
tests/golden/plonk_pi_bn254.json, from the model tests/transcript_expect.py: per case the
verification key's 8 commitments (q_m q_l q_r q_o q_c s_sigma_1..3, from the oracle's
interpolate_at_h and eval_at_s as Plonk.verify forms them), [s]G2's four coordinates, the circuit
digest, the six challenges and t6; then the batch weights of all cases taken as one batch (their
circuits differ: the record fixes the rho formula, not a batch anyone would verify).
Writes tests/golden/plonk_fs_bn254.json."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import plonk_pi_expect as E  # noqa: E402
import transcript_expect as T  # noqa: E402

MODES = {"reference": 0, "paper": 1}


def vk_points(st, q, copies):
    pl = st.plonk
    q_l, q_r, q_o, q_m, q_c = q
    sig = [pl.copy_constraints_to_roots(c) for c in copies]
    return [st.srs.eval_at_s(pl.interpolate_at_h(x)) for x in (q_m, q_l, q_r, q_o, q_c, *sig)]


def g2s_coords(st):
    (x0, x1), (y0, y1) = st.g2_s
    return [int(x0), int(x1), int(y0), int(y1)]


def cases():
    gold = json.load(open(os.path.join(HERE, "plonk_pi_bn254.json")))["cases"]
    out, setups = [], {}
    for c in gold:
        n, npub, mode = c["n"], c["npub"], c["mode"]
        st = setups.setdefault(n, E.setup(n))
        inp = E.case_inputs(n, npub, mode)
        vk = vk_points(st, inp["q"], inp["copies"])
        g2s = g2s_coords(st)
        h0 = T.circuit_digest(MODES[mode], n, npub, 2, 3, vk, g2s)
        pts = [None if p is None or tuple(p) == (0, 0) else tuple(p) for p in c["pts"]]
        ch, t6 = T.proof_chain(h0, inp["pub"], pts, c["fields"])
        out.append({"n": n, "npub": npub, "mode": mode, "vk": [list(p) if p else None for p in vk], "g2s": g2s,
                    "digest": h0.hex(), "challenges": ch, "t6": t6.hex()})
    return out


if __name__ == "__main__":
    cs = cases()
    rhos = T.batch_rhos([bytes.fromhex(c["t6"]) for c in cs])
    with open(os.path.join(HERE, "plonk_fs_bn254.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_plonk_fs_golden.py", "cases": cs,
                   "rhos_of_all_cases_as_one_batch": rhos}, f)
    print([(c["n"], c["npub"], c["mode"], c["digest"][:8]) for c in cs])
