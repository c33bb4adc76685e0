"""CPU test: the protocol's scalar terms of csrc/plonk_terms.hpp (the coefficients of the
linearisation r(x) and of the W_z numerator, which both provers of csrc/prover.hip bind to their
polynomials), compiled for the host, against the polynomials of the literal oracle
(oracle/plonk_bn254.py) at n = 8 in both modes: sum_k c_k p_k must be the oracle's r(x), and
sum_k c_k p_k + c0 must be w_z(x) (x - z), coefficient for coefficient."""
import os
import random
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

N = 8


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plonk_terms")
    path = str(d / "plonk_terms_host_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-w",
                    os.path.join(HERE, "native", "plonk_terms_host_check.hip"), "-o", path], check=True)
    yield path
    shutil.rmtree(d, ignore_errors=True)


def _eval(p, x, R):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def _lincomb(coeffs, polys, R, c0=0):
    out = [0] * max(len(p) for p in polys)
    for c, p in zip(coeffs, polys):
        for i, x in enumerate(p):
            out[i] = (out[i] + c * x) % R
    out[0] = (out[0] + c0) % R
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("mode,seed", [("reference", 11), ("paper", 12)])
def test_plonk_terms_against_oracle_polynomials(exe, tmp_path, mode, seed):
    import plonk_bn254 as P

    R = P.R
    st = P.Setup(N, s=0x5EED0005C0FFEE, srs_n=2 * N + 2)
    q, cp, abc = P.mul_gates_circuit(N, 0x5EED0005 + N)
    rng = random.Random(seed)
    chal = [rng.randrange(R) for _ in range(5)]
    rnd = [rng.randrange(R) for _ in range(9)]
    _, fields, pl = P.prove(st, q, cp, abc, chal, rnd, mode=mode)
    alpha, beta, gamma, z, v = chal
    q_l, q_r, q_o, q_m, q_c = (st.interpolate(col) for col in q)
    l1 = st.interpolate([1] + [0] * (N - 1))
    ev = {"a_z": _eval(pl["a"], z, R), "b_z": _eval(pl["b"], z, R), "c_z": _eval(pl["c"], z, R),
          "s1_z": _eval(pl["s1"], z, R), "s2_z": _eval(pl["s2"], z, R),
          "zw_z": _eval(pl["z"], z * st.omega % R, R), "l1_z": _eval(l1, z, R), "t_z": _eval(pl["t"], z, R),
          "r_z": _eval(pl["r"], z, R)}
    # the evaluations are the proof's own (Proof order: a b c s1 s2 r zw)
    assert [ev[k] for k in ("a_z", "b_z", "c_z", "s1_z", "s2_z", "r_z", "zw_z")] == fields
    ints = [alpha, beta, gamma, z, v, st.k1, st.k2] + [ev[k] for k in ("a_z", "b_z", "c_z", "s1_z", "s2_z", "zw_z",
                                                                          "l1_z", "t_z", "r_z")]
    table = str(tmp_path / "terms.txt")
    with open(table, "w") as f:
        f.write("%d %d\n" % (N, {"reference": 0, "paper": 1}[mode]))
        f.write("\n".join("%064x" % x for x in ints) + "\n")
    out = subprocess.run([exe, table], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [int(l, 16) for l in out.stdout.split()]
    assert len(got) == 17
    rc, wc, c0 = got[:7], got[7:16], got[16]

    seventh = P.pmul(pl["z"], pl["s3"]) if mode == "reference" else pl["s3"]
    r_polys = [q_m, q_l, q_r, q_o, q_c, pl["z"], seventh]
    assert P.norm(_lincomb(rc, r_polys, R)) == pl["r"], "r(x) coefficients"

    w_polys = [pl["t_lo"], pl["t_mid"], pl["t_hi"], pl["r"], pl["a"], pl["b"], pl["c"], pl["s1"], pl["s2"]]
    assert P.norm(_lincomb(wc, w_polys, R, c0)) == P.pmul(pl["w_z"], [(-z) % R, 1]), "W_z numerator"
