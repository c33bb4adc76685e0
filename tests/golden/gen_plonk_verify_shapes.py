#!/usr/bin/env python3
"""Verdicts of the unmodified oracle's verifier (oracle/plonk_bn254.verify through
tests/plonk_pi_expect.verify) at the shapes where the single and the batched GPU verifier are
compared (tests/test_plonk_pi_gpu.py): n = 8 and n = 128, both modes, npub = 0 and 3. The circuit is
plonk_pi_expect.scale_circuit(n, seed), the statement scale_statement(a, b, npub, seed + 1), the
proof the oracle's own. Each case holds its inputs, the proof and four verdicts:
    valid      the proof as it stands (reference mode: rejected)
    a_z        a_z + 1
    off_curve  W_z moved off the curve (y + 1)
    z_omega    z = omega: Z_H(z) = 0, where the reference's unwrap() panics -- recorded as False
The oracle's verifier takes ~13 s per call at n = 128, so the verdicts are recorded here, one
process per case. Writes tests/golden/plonk_verify_shapes.json."""
import json
import multiprocessing
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import plonk_pi_expect as E  # noqa: E402

SHAPES = [(n, npub, mode) for n in (8, 128) for mode in ("reference", "paper") for npub in (0, 3)]


def case(shape):
    n, npub, mode = shape
    seed = 0x5EED1000 + 16 * n + 2 * npub + (mode == "paper")
    st = E.setup(n)
    q, copies, a, b = E.scale_circuit(n, seed)
    pub, abc = E.scale_statement(a, b, npub, seed + 1)
    rng = random.Random(seed + 2)
    chal = [rng.randrange(E.R) for _ in range(5)]
    rnd = [rng.randrange(E.R) for _ in range(9)]
    u = rng.randrange(E.R)
    pts, fs = E.prove(st, q, copies, abc, pub, chal, rnd, mode=mode)

    def verdict(pts=pts, fs=fs, chal=chal):
        try:
            return bool(E.verify(st, q, copies, pub, pts, fs, chal, u, mode=mode))
        except ZeroDivisionError:  # plonk.rs:581 unwrap()
            return False

    off = list(pts)
    off[7] = (off[7][0], (off[7][1] + 1) % E.B.Q)
    verdicts = {"valid": verdict(), "a_z": verdict(fs=[(fs[0] + 1) % E.R] + fs[1:]), "off_curve": verdict(pts=off),
                "z_omega": verdict(chal=chal[:3] + [st.omega] + chal[4:])}
    return {"n": n, "npub": npub, "mode": mode, "seed": seed, "s": E.S_SECRET, "pub": pub, "chal": chal, "u": u,
            "pts": [list(p) if p else None for p in pts], "fields": fs, "verdicts": verdicts}


if __name__ == "__main__":
    with multiprocessing.Pool(min(len(SHAPES), os.cpu_count() or 1)) as pool:
        cs = pool.map(case, SHAPES)
    with open(os.path.join(HERE, "plonk_verify_shapes.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_plonk_verify_shapes.py", "cases": cs}, f)
    print([(c["n"], c["npub"], c["mode"], c["verdicts"]) for c in cs])
