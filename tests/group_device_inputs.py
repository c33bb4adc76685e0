"""Operands and Python models for tests/test_group_device_gpu.py, tests/test_group_device_inputs.py
and the host check of tests/test_field_host.py.

Every point addition of csrc/ec_bn254.hpp and csrc/msm_l29.hpp has four exits (an identity
operand, P + P, P + (-P), the generic formula). The operand tables here are built from known
discrete logs (P = a G by the oracle's g1_mul) so that every exit is entered, in both the
trivial form (the two operands are copies) and the one that needs the cross-multiplied
comparison (two different XYZZ representations of one point: (x l^2, y l^3, l^2, l^3) for
different l). Two references:
  - the group: oracle/bn254.py g1_add / g1_mul on the discrete logs (check_group);
  - integer restatements of the EFD formulas the headers name (madd-2008-s, add-2008-s,
    dbl-2008-s-1, mdbl-2008-s-1; a = 0) with the headers' exits, coordinate for coordinate.
Points are tuples of plain integers mod q: (X, Y, ZZ, ZZZ), ZZ = 0 the identity; affine (x, y).
"""
import os
import functools
import random
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import bn254  # noqa: E402
from field_device_inputs import interleave, u256, from_u256  # noqa: E402,F401

Q, R = bn254.Q, bn254.R
G = bn254.G1_GEN
IDENTITY = (1, 1, 0, 0)  # G1::identity() in plain form
MSM_CH = 43

_PT = {}


def pt(a):
    """a G (None for a = 0 mod r), memoised."""
    a %= R
    if a not in _PT:
        if a and R - a in _PT:
            _PT[a] = neg(_PT[R - a])
        else:
            _PT[a] = bn254.g1_mul(G, a) if a else None
    return _PT[a]


def log_sum(logs):
    """(sum of logs) G as the oracle's fold of g1_add over the points (one inversion per step; a
    g1_mul is several hundred)."""
    acc = None
    for t in logs:
        acc = bn254.g1_add(acc, pt(t))
    return acc


def learn(*logs):
    """The sum of the logs, its point entered into pt()'s table by additions of known points."""
    a = sum(logs) % R
    if a and a not in _PT:
        _PT[a] = log_sum(logs)
    return a


def neg(p):
    return (p[0], (Q - p[1]) % Q)


def lift(p, lam=1):
    """The XYZZ representation (x l^2, y l^3, l^2, l^3) of an affine point."""
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return (p[0] * l2 % Q, p[1] * l3 % Q, l2, l3)


def affine_of(p):
    """The canonical affine point of an XYZZ tuple (None: the identity)."""
    if p[2] == 0:
        return None
    return (p[0] * pow(p[2], Q - 2, Q) % Q, p[1] * pow(p[3], Q - 2, Q) % Q)


def group_ok(out, want):
    """The first check of a device result: the identity (ZZ = 0) where the group says so, else
    every coordinate below q, ZZ != 0, ZZ^3 = ZZZ^2 and (X / ZZ, Y / ZZZ) the expected point."""
    X, Y, ZZ, ZZZ = out
    if want is None:
        return ZZ == 0
    return (max(out) < Q and ZZ != 0 and pow(ZZ, 3, Q) == ZZZ * ZZZ % Q
            and X == want[0] * ZZ % Q and Y == want[1] * ZZZ % Q)


# ---- the formulas, as the headers state them ------------------------------------------------------
# wrong: one deliberately wrong exit (tests/test_group_device_inputs.py):
#   "no_p0"   the P = 0 test dropped (the generic formula runs on equal and opposite operands)
#   "y_plain" P + P told from P + (-P) by the operands' own Y, not cross-multiplied
#   "id_x"    is_identity reading X instead of ZZ
def is_identity(p, wrong=None):
    return p[0] == 0 if wrong == "id_x" else p[2] == 0


def mdbl(a):
    x, y = a
    U = 2 * y % Q
    V = U * U % Q
    W = U * V % Q
    S = x * V % Q
    M = 3 * x * x % Q
    X3 = (M * M - 2 * S) % Q
    return (X3, (M * (S - X3) - W * y) % Q, V, W)


def dbl(p, wrong=None):
    if is_identity(p, wrong):
        return p
    X, Y, ZZ, ZZZ = p
    U = 2 * Y % Q
    V = U * U % Q
    W = U * V % Q
    S = X * V % Q
    M = 3 * X * X % Q
    X3 = (M * M - 2 * S) % Q
    return (X3, (M * (S - X3) - W * Y) % Q, V * ZZ % Q, W * ZZZ % Q)


def madd(p, a, wrong=None):
    if is_identity(p, wrong):
        return (a[0], a[1], 1, 1)
    X, Y, ZZ, ZZZ = p
    P = (a[0] * ZZ - X) % Q
    Rr = (a[1] * ZZZ - Y) % Q
    if P == 0 and wrong != "no_p0":
        same = a[1] == Y if wrong == "y_plain" else Rr == 0
        return mdbl(a) if same else IDENTITY
    PP = P * P % Q
    PPP = P * PP % Q
    Qq = X * PP % Q
    X3 = (Rr * Rr - PPP - 2 * Qq) % Q
    return (X3, (Rr * (Qq - X3) - Y * PPP) % Q, ZZ * PP % Q, ZZZ * PPP % Q)


def add(p, q, wrong=None):
    if is_identity(p, wrong):
        return q
    if is_identity(q, wrong):
        return p
    U1, U2 = p[0] * q[2] % Q, q[0] * p[2] % Q
    S1, S2 = p[1] * q[3] % Q, q[1] * p[3] % Q
    P, Rr = (U2 - U1) % Q, (S2 - S1) % Q
    if P == 0 and wrong != "no_p0":
        same = p[1] == q[1] if wrong == "y_plain" else Rr == 0
        return dbl(p, wrong) if same else IDENTITY
    PP = P * P % Q
    PPP = P * PP % Q
    Qq = U1 * PP % Q
    X3 = (Rr * Rr - PPP - 2 * Qq) % Q
    return (X3, (Rr * (Qq - X3) - S1 * PPP) % Q, p[2] * q[2] % Q * PP % Q, p[3] * q[3] % Q * PPP % Q)


def mul_small(p, k):
    r = IDENTITY
    for b in range(k.bit_length() - 1, -1, -1):
        r = dbl(r)
        if (k >> b) & 1:
            r = add(r, p)
    return r


def chain(points):
    """The accumulation of msm_chunk_acc_l29r over affine points, through madd: the point, the
    mask of the steps that took the doubling exit and the mask of the steps that left the
    identity."""
    acc, dbl_mask, id_mask = IDENTITY, 0, 0
    for j, a in enumerate(points):
        if acc[2] != 0 and (a[0] * acc[2] - acc[0]) % Q == 0 and (a[1] * acc[3] - acc[1]) % Q == 0:
            dbl_mask |= 1 << j
        acc = madd(acc, a)
        if acc[2] == 0:
            id_mask |= 1 << j
    return acc, dbl_mask, id_mask


def chain_masks_from_logs(logs):
    """The same two masks predicted from the discrete logs alone."""
    acc, dbl_mask, id_mask = 0, 0, 0
    for j, t in enumerate(logs):
        t %= R
        assert t
        if acc and acc == t:
            dbl_mask |= 1 << j
        acc = (acc + t) % R
        if acc == 0:
            id_mask |= 1 << j
    return dbl_mask, id_mask


# ---- operands ---------------------------------------------------------------------------------------
_RND = random.Random(0x61C0)
LOGS = [1, R - 1, 2, R - 2] + [_RND.randrange(3, R - 2) for _ in range(12)]
PAIR_KINDS = ("generic", "eq_same", "eq_diff", "neg_same", "neg_diff", "p_id", "q_id", "both_id")
MIXED_KINDS = ("generic", "eq_same", "eq_diff", "neg_same", "neg_diff", "p_id")

# a, b: the discrete logs of the operands (0: the identity); kind: one of PAIR_KINDS / MIXED_KINDS
Case = namedtuple("Case", "kind p q a b")


def _lam(rnd):
    return rnd.randrange(2, Q)


def _junk_identity(rnd):
    """ZZ = ZZZ = 0 with arbitrary X, Y: is_identity reads ZZ only."""
    return (rnd.randrange(1, Q), rnd.randrange(Q), 0, 0)


def _identities(rnd):
    return [IDENTITY, _junk_identity(rnd), _junk_identity(rnd)]


@functools.lru_cache(maxsize=None)
def pair_cases_chosen():
    """XYZZ + XYZZ: every kind in several instances; a = 1 (G = (1, 2), small coordinates) and
    a = r - 1 are the first logs, in every kind."""
    rnd = random.Random(0x9A11)
    out = []
    for i, a in enumerate(LOGS):
        b = LOGS[(i + 5) % len(LOGS)]
        if (a + b) % R == 0 or a == b:
            b = LOGS[(i + 6) % len(LOGS)]
        P, Bq = pt(a), pt(b)
        l1, l2 = _lam(rnd), _lam(rnd)
        out.append(Case("generic", lift(P, l1), lift(Bq, l2), a, b))
        out.append(Case("generic", lift(P), lift(Bq), a, b))
        out.append(Case("eq_same", lift(P, l1), lift(P, l1), a, a))
        out.append(Case("eq_same", lift(P), lift(P), a, a))
        out.append(Case("eq_diff", lift(P, l1), lift(P, l2), a, a))
        out.append(Case("eq_diff", lift(P), lift(P, l2), a, a))
        out.append(Case("eq_diff", lift(P, l1), lift(P), a, a))
        out.append(Case("neg_same", lift(P, l1), lift(neg(P), l1), a, R - a))
        out.append(Case("neg_same", lift(P), lift(neg(P)), a, R - a))
        out.append(Case("neg_diff", lift(P, l1), lift(neg(P), l2), a, R - a))
        out.append(Case("neg_diff", lift(neg(P)), lift(P, l2), R - a, a))
        for ident in _identities(rnd):
            out.append(Case("p_id", ident, lift(P, l1), 0, a))
            out.append(Case("q_id", lift(P, l2), ident, a, 0))
    for p in _identities(rnd):
        for q in _identities(rnd):
            out.append(Case("both_id", p, q, 0, 0))
    return out


def pair_cases_random(n=150, seed=0x9A12):
    """Random points in random representations: the generic exit only."""
    rnd = random.Random(seed)
    logs = LOGS[4:]
    out = []
    for _ in range(n):
        a, b = rnd.sample(logs, 2)
        out.append(Case("generic", lift(pt(a), _lam(rnd)), lift(pt(b), _lam(rnd)), a, b))
    return out


@functools.lru_cache(maxsize=None)
def pair_cases():
    return interleave(pair_cases_chosen() + pair_cases_random(40))


@functools.lru_cache(maxsize=None)
def mixed_cases_chosen():
    """XYZZ accumulator + affine point (never the identity). eq_diff / neg_diff: the affine
    operand equal / opposite to an accumulator in a non-trivial representation."""
    rnd = random.Random(0x9A13)
    out = []
    for i, a in enumerate(LOGS):
        b = LOGS[(i + 3) % len(LOGS)]
        if (a + b) % R == 0 or a == b:
            b = LOGS[(i + 4) % len(LOGS)]
        P, Bq = pt(a), pt(b)
        l1 = _lam(rnd)
        out.append(Case("generic", lift(P, l1), Bq, a, b))
        out.append(Case("generic", lift(P), Bq, a, b))
        out.append(Case("eq_same", lift(P), P, a, a))
        out.append(Case("eq_diff", lift(P, l1), P, a, a))
        out.append(Case("eq_diff", lift(P, _lam(rnd)), P, a, a))
        out.append(Case("neg_same", lift(P), neg(P), a, R - a))
        out.append(Case("neg_diff", lift(P, l1), neg(P), a, R - a))
        out.append(Case("neg_diff", lift(neg(P), _lam(rnd)), P, R - a, a))
        for ident in _identities(rnd):
            out.append(Case("p_id", ident, P, 0, a))
    return out


def mixed_cases_random(n=150, seed=0x9A14):
    rnd = random.Random(seed)
    logs = LOGS[4:]
    out = []
    for _ in range(n):
        a, b = rnd.sample(logs, 2)
        out.append(Case("generic", lift(pt(a), _lam(rnd)), pt(b), a, b))
    return out


@functools.lru_cache(maxsize=None)
def mixed_cases():
    return interleave(mixed_cases_chosen() + mixed_cases_random(40))


@functools.lru_cache(maxsize=None)
def unary_cases():
    """(point, log): every log in the affine lift and two random representations, and the
    identities (log 0)."""
    rnd = random.Random(0x9A15)
    out = []
    for a in LOGS:
        out += [(lift(pt(a)), a), (lift(pt(a), _lam(rnd)), a), (lift(pt(a), _lam(rnd)), a)]
    for _ in range(3):
        out += [(p, 0) for p in _identities(rnd)]
    return interleave(out)


def kinds(cases, names):
    got = {k: 0 for k in names}
    for c in cases:
        got[c.kind] += 1
    return got


def exit_of(c):
    """The exit an addition takes on a case: 'id', 'dbl', 'opp' or 'generic'."""
    if c.kind in ("p_id", "q_id", "both_id"):
        return "id"
    return {"eq": "dbl", "ne": "opp", "ge": "generic"}[c.kind[:2]]


# ---- chains: K affine points by their discrete logs ---------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_cases():
    """{K: [(name, logs)]}: the accumulation step's exits in sequence (Q, S, T distinct from +-P)."""
    rnd = random.Random(0x9A16)
    P, Qq, S, T = LOGS[4], LOGS[5], LOGS[6], LOGS[7]
    out = {1: [], 2: [], 3: [], 5: [], MSM_CH: []}
    for a in LOGS[:8]:
        out[1].append(("single", [a]))
        out[2].append(("P P", [a, a]))
        out[2].append(("P -P", [a, R - a]))
    out[2].append(("P Q", [P, Qq]))
    S1, T1 = learn(S, 1), learn(T, 1)
    for p, q in [(P, Qq), (1, S), (R - 1, T), (S, 2), (T, R - 2), (Qq, 1)]:
        pq, p2, rest = learn(p, q), learn(p, p), learn(p, q, S1, T1)
        out[3].append(("P -P Q", [p, R - p, q]))
        out[3].append(("P P P", [p, p, p]))
        out[3].append(("P Q P+Q", [p, q, pq]))
        out[3].append(("P Q -(P+Q)", [p, q, R - pq]))
        out[3].append(("P P 2P", [p, p, p2]))
        out[3].append(("P P -2P", [p, p, R - p2]))
        out[3].append(("P Q S", [p, q, learn(p2, p, q)]))
        out[5].append(("exceptional first", [p, p, q, S1, T1]))
        out[5].append(("exceptional middle", [p, q, pq, S1, T1]))
        out[5].append(("exceptional last", [p, q, S1, T1, rest]))
        out[5].append(("identity middle, fresh run", [p, q, R - pq, S1, S1]))
        out[5].append(("identity last", [p, q, S1, T1, R - rest]))
    pool = [rnd.randrange(1 << 40, 1 << 48) for _ in range(MSM_CH)]  # short logs: a quick g1_mul each
    for a in (P, 1, R - 1, Qq):
        out[MSM_CH].append(("43 copies", [a] * MSM_CH))
    out[MSM_CH].append(("43 distinct", pool))
    out[MSM_CH].append(("43 distinct, reversed", pool[::-1]))
    for where in (1, 21, 42):  # the exceptional step first, in the middle, last
        logs = list(pool)
        logs[where] = learn(*logs[:where])
        out[MSM_CH].append(("exceptional at %d" % where, logs))
        logs = list(pool)
        logs[where] = R - learn(*logs[:where])
        out[MSM_CH].append(("identity at %d" % where, logs))
    alt = [P, R - P] * 21 + [P]
    out[MSM_CH].append(("alternating P -P", alt))
    for k in out:
        assert all(len(logs) == k for _, logs in out[k])
        items = out[k]
        random.Random(k).shuffle(items)
        out[k] = [(n, [t % R for t in logs]) for n, logs in items]
    return out


# ---- packing ----------------------------------------------------------------------------------------
def pack(points):
    """Tuples of plain integers -> (n, 4 * len(tuple)) uint64."""
    flat = [v for p in points for v in p]
    return u256(flat).reshape(len(points), -1)


def unpack(arr, width):
    """(n, 4 * width) uint64 -> n tuples of `width` integers."""
    vals = from_u256(arr)
    return [tuple(vals[i:i + width]) for i in range(0, len(vals), width)]


# ---- the case table of tests/native/g1_host_check.hip ------------------------------------------------
MUL_SMALL_KS = (0, 1, 2, 3, 5, 8, 255, 0x10001, 0xFFFFFFFF)


def to_affine_ref(p):
    """to_affine_plain: the canonical affine point, (0, 0) for the identity."""
    a = affine_of(p)
    return (0, 0) if a is None else a


def host_case_lines():
    """One line per case: op, k, then inputs and the formula models' outputs as 64 hex digits."""
    def line(op, k, *points):
        return "%s %d %s" % (op, k, " ".join("%064x" % v for p in points for v in p))

    out = []
    for c in pair_cases():
        r = add(c.p, c.q)
        out += [line("add", 0, c.p, c.q, r), line("add2", 0, c.p, c.q, r)]
    for c in mixed_cases():
        r = madd(c.p, c.q)
        out += [line("madd", 0, c.p, c.q, r), line("madd_tp", 0, c.p, c.q, r)]
    for p, a in unary_cases():
        r = dbl(p)
        out += [line("dbl", 0, p, r), line("dbl2", 0, p, r), line("to_affine", 0, p, to_affine_ref(p))]
        if a:
            out.append(line("mdbl", 0, pt(a), mdbl(pt(a))))
        out += [line("mul_small", k, p, mul_small(p, k)) for k in MUL_SMALL_KS]
    return out
