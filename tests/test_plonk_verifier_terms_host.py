"""CPU test: Plonk::verify's steps 4-10 as csrc/plonk_terms.hpp states them once for the single
verifier (csrc/verify.hip, rho = 1) and the batched kernel (csrc/verify_batch.hip k_vb_scalars):
plonk_verifier_scalars and plonk_domain, compiled for the host, value by value against plain Python
arithmetic mod r that follows oracle/plonk.py Plonk.verify lines 348-381 (steps 4-11: z_h_z, l_1_z,
perm, t_z, the scalars of d_1_s, d_2_s, d_3_s, f_s, e_s, e_1_q1 and e_2_q1). L_1(z) is the oracle's
interpolation of [1, 0, ...] on H (oracle/plonk_bn254.py Setup.interpolate) evaluated at z, Z_H(z)
the oracle's z_h_x, omega the oracle's; no closed form. With a fraction (N, D) of the public inputs
p_i_z, 0 in the oracle, is PI(z) = -Z_H(z) N / (n D) (include/pbf.h "Public inputs").

n = 8 and n = 128, both modes, rho = 1 and random, no fraction and a random one, on seeded random
challenges and evaluations; and z = omega, where the function must report Z_H(z) = 0."""
import os
import random
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

CASES = [(n, mode, rho_one, frac) for n in (8, 128) for mode in (0, 1) for rho_one in (True, False)
         for frac in (False, True)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plonk_verifier_terms")
    path = str(d / "plonk_verifier_terms_host_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-w",
                    os.path.join(HERE, "native", "plonk_verifier_terms_host_check.hip"), "-o", path], check=True)
    yield path
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def setups():
    """The oracle's domain per n (no SRS needed: srs_n = 0), with L_1(x) interpolated once."""
    import plonk_bn254 as P

    out = {}
    for n in (8, 128):
        st = P.Setup(n, s=0x5EED0005C0FFEE, srs_n=0)
        out[n] = (st, st.interpolate([1] + [0] * (n - 1)))
    return out


def _eval(p, x, R):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def _expected(R, n, omega, z_h_z, l_1_z, mode, chal, k1, k2, fields, u, rho, nd):
    """The 20 scalars in the order of plonk_verifier_scalars' out(j, .), from oracle/plonk.py lines 348-381."""
    alpha, beta, gamma, z, v = chal
    a_z, b_z, c_z, s1_z, s2_z, r_z, zw_z = fields
    p_i_z = 0 if nd is None else -z_h_z * nd[0] * pow(n * nd[1], -1, R)
    perm = (beta * s1_z + gamma + a_z) * (beta * s2_z + gamma + b_z) * (c_z + gamma) * zw_z  # line 353
    if mode == 1:
        perm *= alpha
    t_z = (r_z + p_i_z - perm - l_1_z * pow(alpha, 2, R)) * pow(z_h_z, -1, R) % R  # line 358
    d_2 = ((a_z + beta * z + gamma) * (b_z + beta * k1 * z + gamma) * (c_z + beta * k2 * z + gamma) * alpha * v
           + l_1_z * pow(alpha, 2, R) * v + u) % R  # lines 362-363
    d_3 = (a_z + beta * s1_z + gamma) * (b_z + beta * s2_z + gamma) * alpha * v * beta * zw_z % R  # lines 364-365
    e = (t_z + v * r_z + pow(v, 2, R) * a_z + pow(v, 3, R) * b_z + pow(v, 4, R) * c_z + pow(v, 5, R) * s1_z
         + pow(v, 6, R) * s2_z + u * zw_z) % R  # lines 376-378
    proof = [pow(v, 2, R), pow(v, 3, R), pow(v, 4, R), d_2, 1, pow(z, n + 2, R), pow(z, 2 * n + 4, R), z,
             u * z * omega]  # lines 373-374, 362, 369-371, 381
    e1 = [1, u]  # line 380
    shared = [v * a_z * b_z, v * a_z, v * b_z, v * c_z, v, pow(v, 5, R), pow(v, 6, R), -d_3, -e]  # lines 360-361, 373-378
    return [rho * x % R for x in proof + e1 + shared]


def _run(exe, path, n, mode, ints, nd):
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (n, mode, nd is not None))
        f.write("\n".join("%064x" % x for x in ints + list(nd or ())) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("n,mode,rho_one,frac", CASES,
                         ids=["n%d-mode%d-%s-%s" % (n, m, "rho1" if r else "rho", "pi" if f else "plain")
                              for n, m, r, f in CASES])
def test_verifier_scalars_against_the_oracles_formulas(exe, setups, tmp_path, n, mode, rho_one, frac):
    import plonk_bn254 as P

    R = P.R
    st, l1 = setups[n]
    rng = random.Random(1000 * n + 100 * mode + 10 * rho_one + frac)
    chal = [rng.randrange(R) for _ in range(5)]
    fields = [rng.randrange(R) for _ in range(7)]
    u = rng.randrange(R)
    rho = 1 if rho_one else rng.randrange(1, R)
    nd = (rng.randrange(R), rng.randrange(1, R)) if frac else None
    z = chal[3]
    z_h_z = st.plonk.z_h_x.eval(z) % R
    assert z_h_z != 0
    want = _expected(R, n, st.omega, z_h_z, _eval(l1, z, R), mode, chal, st.k1, st.k2, fields, u, rho, nd)
    got = _run(exe, str(tmp_path / "in.txt"), n, mode, chal + [st.k1, st.k2] + fields + [u, rho], nd)
    got = [int(x, 16) for x in got.split()]
    assert len(got) == 20
    names = "a b c z t_lo t_mid t_hi w_z w_zw e1_wz e1_wzw q_m q_l q_r q_o q_c s1 s2 s3 G".split()
    assert {k: x for k, x in zip(names, got)} == {k: x for k, x in zip(names, want)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("frac", [False, True], ids=["plain", "pi"])
def test_z_in_h_is_reported_and_nothing_is_handed_out(exe, setups, tmp_path, frac):
    import plonk_bn254 as P

    R = P.R
    st, _ = setups[8]
    rng = random.Random(88 + frac)
    chal = [rng.randrange(R) for _ in range(5)]
    chal[3] = st.omega
    assert st.plonk.z_h_x.eval(chal[3]) % R == 0
    ints = chal + [st.k1, st.k2] + [rng.randrange(R) for _ in range(7)] + [rng.randrange(R), rng.randrange(1, R)]
    # z in H makes D = 0 too (csrc/verify_batch.hip k_vb_pi_*); the fraction must not be read
    got = _run(exe, str(tmp_path / "in.txt"), 8, 1, ints, (rng.randrange(R), 0) if frac else None)
    assert got == "Z_H(z) = 0\n"
