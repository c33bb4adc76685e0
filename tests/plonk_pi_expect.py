"""Expected values of the public-input prover and verifiers (include/pbf.h "Public inputs") from the
unmodified oracle (oracle/plonk_bn254.py), which knows no public inputs.

Public input i < npub sits on gate row i: PI(w^i) = -pub_i, 0 on the other rows, PI(x) its
interpolation on H, and the gate equation is q_l a + q_r b + q_o c + q_m a b + q_c + PI = 0 on H.
PI(x) enters the quotient's t_1 only; r(x) keeps q_c(x) and gains no PI term.

Let q' be q with q_c'[i] = q_c[i] - pub_i for i < npub, so q_c'(x) = q_c(x) + PI(x). The oracle's
prover on q' forms the same quotient t(x) (its t_1 holds q_c'(x)), the same a b c z and the same
evaluations; only its linearisation differs, r'(x) = r(x) + PI(x) (plonk.rs:401-419: the q_c term
enters r with coefficient 1). Hence, from the oracle's proof (') on q':
    r_z = r_z' - PI(z)
    W_z = W_z' - [v] commit((PI(x) - PI(z)) / (x - z))      (plonk.rs:424-438: v (r(x) - r_z))
and the other 8 points and 6 fields are the same. The map (r_z, W_z) <-> (r_z', W_z') is a bijection
for fixed (pub, z, v), and the verifier's equation is the same one under it: step 7 reads r_z + PI(z)
= r_z' where the oracle reads r_z', [v r_z]G and z W_z move by the same amounts on both sides. So "the
_pi verifier accepts (proof, pub) for q" is exactly "plonk_bn254.verify accepts to_oracle(proof, pub)
for q'", for acceptance and for rejection.

PI, its quotient and the commitment come from Setup.interpolate, pdiv and Setup.eval_at_s.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254_pairing as B  # noqa: E402
import plonk_bn254 as P  # noqa: E402

R = P.R


def q_prime(q, pub):
    """q with q_c'[i] = q_c[i] - pub_i on rows i < npub."""
    qc = list(q[4])
    for i, x in enumerate(pub):
        qc[i] = (qc[i] - x) % R
    return (q[0], q[1], q[2], q[3], qc)


def pi_poly(st, pub):
    """Coefficients of PI(x): the interpolation of -pub_i on rows i < npub, 0 elsewhere."""
    return st.interpolate([(-x) % R for x in pub] + [0] * (st.n - len(pub)))


def poly_eval(c, x):
    y = 0
    for v in reversed(c):
        y = (y * x + v) % R
    return y


def pi_opening(st, pub, z):
    """(PI(z), commit((PI(x) - PI(z)) / (x - z)))."""
    c = pi_poly(st, pub)
    y = poly_eval(c, z)
    num = P.norm([((c[0] if c else 0) - y) % R] + list(c[1:]))
    quo, rem = P.pdiv(num, [(-z) % R, 1]) if num else ([], [])
    assert rem == []
    return y, (st.eval_at_s(quo) if quo else None)


def _shift(st, pub, chal, pts, fs, sign):
    z, v = chal[3] % R, chal[4] % R
    y, com = pi_opening(st, pub, z)
    pts, fs = [None if p is None else tuple(p) for p in pts], list(fs)
    fs[5] = (fs[5] + sign * y) % R
    pts[7] = B.g1_add(pts[7], B.g1_mul(com, sign * v % R))
    return pts, fs


def from_oracle(st, pub, chal, pts, fs):
    """The public-input proof for (q, pub) from the oracle's proof for q'."""
    return _shift(st, pub, chal, pts, fs, -1)


def to_oracle(st, pub, chal, pts, fs):
    """The proof the oracle's verifier must be shown for q' = q_prime(q, pub)."""
    return _shift(st, pub, chal, pts, fs, 1)


def prove(st, q, copies, abc, pub, chal, rnd, mode="reference"):
    pts, fs, _ = P.prove(st, q_prime(q, pub), copies, abc, chal, rnd, mode=mode)
    return from_oracle(st, pub, chal, pts, fs)


def verify(st, q, copies, pub, pts, fs, chal, u, mode="reference"):
    po, fo = to_oracle(st, pub, chal, pts, fs)
    return P.verify(st, q_prime(q, pub), copies, po, fo, chal, u, mode=mode)


# ---------------------------------------------------------------- circuits
def small_circuit(n, npub, seed):
    """Even rows i < npub are classic public rows (q_l = 1, a_i = pub_i, b_i = c_i = 0), odd rows
    i < npub multiplication gates that carry a public input (c_i = a_i b_i - pub_i), the rest
    plain multiplication gates. Row 0's a wire (= pub_0) is copy-constrained to a_1, the a wire of
    the first multiplication gate. Passes the reference's pre-check with its q_l * b term, since
    b = 0 wherever q_l = 1. Returns q, copies, abc, pub."""
    rng = random.Random(seed)
    pub = [rng.randrange(R) for _ in range(npub)]
    a = [rng.randrange(R) for _ in range(n)]
    b = [rng.randrange(R) for _ in range(n)]
    c = [0] * n
    ql, qo, qm = [0] * n, [0] * n, [0] * n
    a[1] = pub[0]
    for i in range(n):
        if i < npub and i % 2 == 0:
            ql[i], a[i], b[i], c[i] = 1, pub[i], 0, 0
        else:
            qm[i], qo[i] = 1, R - 1
            c[i] = (a[i] * b[i] - (pub[i] if i < npub else 0)) % R
    q = (ql, [0] * n, qo, qm, [0] * n)
    c_a = [(0, i + 1) for i in range(n)]
    c_a[0], c_a[1] = (0, 2), (0, 1)
    copies = (c_a, [(1, i + 1) for i in range(n)], [(2, i + 1) for i in range(n)])
    return q, copies, (a, b, c), pub


def scale_circuit(n, seed):
    """oracle mul_gates_circuit: one circuit (q, copies) and its a, b wires, for any number of
    statements (scale_statement)."""
    q, copies, (a, b, _c) = P.mul_gates_circuit(n, seed)
    return q, copies, a, b


def scale_statement(a, b, npub, seed, fixed=()):
    """A statement of scale_circuit: c_i = a_i b_i - pub_i on rows i < npub, c_i = a_i b_i after
    them; a row i % 4 == 0 hands its c on to a_(i+1), the wire it is tied to, so the witness
    follows the statement. pub is uniform; fixed: (row, value) pairs that override it. One circuit
    and arbitrarily many distinct statements. Returns pub, abc."""
    rng = random.Random(seed)
    n = len(a)
    pub = [rng.randrange(R) for _ in range(npub)]
    for i, v in fixed:
        if 0 <= i < npub:
            pub[i] = v % R
    a, c = list(a), [0] * n
    for i in range(n):
        c[i] = (a[i] * b[i] - (pub[i] if i < npub else 0)) % R
        if i % 4 == 0 and i + 1 < n:
            a[i + 1] = c[i]
    return pub, (a, list(b), c)


# ---------------------------------------------------------------- fixture cases
S_SECRET = 0x5EED0005C0FFEE
CASES = [(8, 1), (8, 2), (16, 5), (16, 16)]  # (n, npub), each in both modes


def case_inputs(n, npub, mode):
    """Everything a fixture case is made from, from its (n, npub, mode) alone."""
    seed = 0x5EED0F1 + 64 * n + 2 * npub + (mode == "paper")
    q, copies, abc, pub = small_circuit(n, npub, seed)
    rng = random.Random(seed + 1)
    chal = [rng.randrange(R) for _ in range(5)]
    rnd = [rng.randrange(R) for _ in range(9)]
    return {"q": q, "copies": copies, "abc": abc, "pub": pub, "chal": chal, "rnd": rnd, "u": 0x1234567,
            "s": S_SECRET, "srs_n": 2 * n + 2}


def setup(n):
    return P.Setup(n, s=S_SECRET, srs_n=2 * n + 2)
