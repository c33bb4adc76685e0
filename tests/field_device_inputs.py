"""Operand sets, case classifiers and integer references for the device field arithmetic tests.

Shared by tests/test_field_device_gpu.py (which runs the operands through the device code of
csrc/field.hpp, fp256.hpp, fr29.hpp, msm_l29.hpp, ntt_kernels.hpp and ntt_gl.hpp) and
tests/test_field_device_inputs.py (which checks, on the CPU, that the operands reach every
branch of those functions and would expose a wrong one). Nothing here touches a GPU.

The classifiers mirror the CASE SPLITS of the device code (which correction a lane takes), not
its instructions; the references are plain Python integer arithmetic.
"""
import random

import numpy as np

GOLD = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M64 = (1 << 64) - 1
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R256 = 1 << 256
R261 = 1 << 261

# the edge values of tests/test_ntt_gpu.py (EDGE_GL), then p >> 1 and 2^64 - 2^32 - 1
EDGE_GL = [0, 1, 2, GOLD - 1, GOLD - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 63) - 1,
           GOLD - (1 << 32), GOLD - (1 << 32) + 1, (1 << 64) - (1 << 33), 0xFFFFFFFE00000001, 0x00000000FFFFFFFF,
           0x7FFFFFFF80000000]
GL_VALUES = EDGE_GL + [GOLD >> 1, 0xFFFFFFFEFFFFFFFF]

MOD32_MODULI = [3, 337, 65537, 3221225473, (1 << 31) - 1, (1 << 31) + 11, (1 << 32) - 5, (1 << 32) - 1]


def interleave(items, seed=0x5EED):
    """A fixed permutation (not a sort): neighbouring lanes get operands of unrelated origin, so
    the per-lane carry masks of one wave mix the cases. The length is then made no multiple of
    64 (the last wave is partial) by repeating leading items."""
    items = list(items)
    random.Random(seed).shuffle(items)
    k = 0
    while len(items) % 64 in (0, 1):
        items.append(items[k])
        k += 1
    return items


# ---- Goldilocks ---------------------------------------------------------------------------------
RED96_CASES = ("plain", "c1", "ge", "both", "c2")


def red96_case(lo, h0, h1):
    """The case gl_red96 takes for lo + h0 2^64 + h1 2^96: c1 = carry of lo + h0 EPS, c2 = borrow
    of - h1. c1 only: + EPS; c2 only: - EPS; both or neither: - p when r >= p (both always is)."""
    s = lo + h0 * EPS
    c1 = s >> 64
    r = s & M64
    c2 = r < h1
    r = (r - h1) & M64
    if c1 and c2:
        return "both"
    if c1:
        return "c1"
    if c2:
        return "c2"
    return "ge" if r >= GOLD else "plain"


def red96_low_word_case(lo, h0, h1):
    """The sub-branch of gl_red96's final correction: the correction is applied to the low word
    and its borrow / carry (lane masks c3 / c4) moves the high word. "c3": a + EPS correction
    (cases c1, ge, both: - p = + EPS mod 2^64) whose low word is 0; "c4": the - EPS correction
    whose low word is 0xFFFFFFFF; else None."""
    case = red96_case(lo, h0, h1)
    low = (lo + h0 * EPS - h1) & EPS
    if case in ("c1", "ge", "both") and low == 0:
        return "c3"
    if case == "c2" and low == EPS:
        return "c4"
    return None


def low_word_counts(args):
    subs = [red96_low_word_case(*a) for a in args]
    return {"c3": subs.count("c3"), "c4": subs.count("c4")}


def red96_model(lo, h0, h1, drop=None):
    """gl_red96 by its case split. drop = a case name: that case's correction is left out (a
    deliberately wrong model, tests/test_field_device_inputs.py)."""
    s = lo + h0 * EPS
    r = ((s & M64) - h1) & M64
    case = red96_case(lo, h0, h1)
    if case == drop:
        return r
    if case == "c1":
        return (r + EPS) & M64
    if case == "c2":
        return (r - EPS) & M64
    if case in ("ge", "both"):
        return (r - GOLD) & M64
    return r


def mul_red96_args(a, b):
    t = a * b
    return t & M64, (t >> 64) & 0xFFFFFFFF, t >> 96


def mul_pow2_red96_args(x, s):
    """Goldilocks::mul_pow2<S> reaches reduce128 (gl_red96) only for 32 < S < 64: S <= 32 and both
    steps of S >= 64 go through add_mul_eps."""
    assert 32 < s < 64
    hi = x >> (64 - s)
    return (x << s) & M64, hi & 0xFFFFFFFF, hi >> 32


ADDMUL_CASES = ("plain", "carry", "ge")


def addmul_eps_case(lo, h):
    s = lo + h * EPS
    if s >> 64:
        return "carry"
    return "ge" if s >= GOLD else "plain"


def count_cases(cases, names):
    out = {n: 0 for n in names}
    for c in cases:
        out[c] += 1
    return out


def gl_random(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(GOLD) for _ in range(n)]


def gl_pairs_chosen():
    """All ordered pairs of GL_VALUES and the family (x 2^48, y 2^48), 0 < x, y < 2^16, whose
    products always take the c2-only (- EPS) correction."""
    pairs = [(a, b) for a in GL_VALUES for b in GL_VALUES]
    rng = random.Random(48)
    xs = [1, 2, 3, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF] + [rng.randrange(1, 1 << 16) for _ in range(9)]
    pairs += [(x << 48, y << 48) for x in xs for y in xs]
    # a b = 2^96 exactly: r = 2^64 - 1, the - EPS correction carries out of the low word (c4)
    pairs += [(1 << k, 1 << (96 - k)) for k in range(33, 64, 3)]
    return pairs


def gl_pairs_random(n=3000, seed=0x61):
    v = gl_random(2 * n, seed)
    return list(zip(v[:n], v[n:]))


def gl_pairs():
    return interleave(gl_pairs_chosen() + gl_pairs_random())


def gl_unary_chosen():
    """GL_VALUES, every power of two (x = 2^(96-S) is the one kind of operand for which
    mul_pow2<S>, 32 < S < 64, borrows without a carry), and k 2^32 + 2^j - k (for j = 64 - S and
    small k the sum lands in [p, 2^64) without a carry)."""
    v = GL_VALUES + [1 << k for k in range(64)]
    v += [(k << 32) + (1 << j) - k for k in (1, 2, 3, 4) for j in range(1, 32) if 1 << j >= k]  # k = 1: as above
    # 2^(97-S) - 1: a carry, then the + EPS correction borrows out of a zero low word (c3)
    v += [(1 << k) - 1 for k in range(2, 64)]
    v += [h << k for h in (3, 5, 7, 0xFFFF) for k in range(64) if h << k < GOLD]  # h1 2^(96-S), other h1
    return v


def gl_unary():
    return interleave(gl_unary_chosen() + gl_random(3000, 0x62))


# Which gl_red96 cases mul_pow2<S> can reach, 32 < S < 64, for canonical x = hi 2^(64-S) + xl:
# lo = xl 2^S, h0 + 2^32 h1 = hi < 2^S.
#   c2 only needs lo + h0 EPS < h1 < 2^(S-32): lo = 0, h0 = 0, h1 > 0, i.e. x = h1 2^(96-S).
#   both needs lo + h0 EPS = 2^64 + t with t < h1: mod 2^32, h0 = 2^32 - t, so lo = 2^32 (1 + t),
#     a multiple of 2^S only for t >= 2^(S-32) - 1 >= h1: never.
#   ge: x = 2^32 + 2^(64-S) - 1 gives lo = 2^64 - 2^S, h0 = 2^(S-32), h1 = 0, r = 2^64 - 2^(S-32).
# The same for every S of the range; tests/test_field_device_inputs.py recomputes it from
# gl_unary() and compares.
MUL_POW2_REACH = {s: ("plain", "c1", "ge", "c2") for s in range(33, 64)}


def reduce128_pairs():
    """(lo, hi), arbitrary 64-bit words: every pair of the edge words, one construction per case,
    random words."""
    words = GL_VALUES + [M64, M64 - 1, GOLD, GOLD + 1, 1 << 33, (1 << 64) - (1 << 32)]
    pairs = [(a, b) for a in words for b in words]
    pairs += [(0, 1 << 32), (5, 7 << 32), (M64, 1), (M64, EPS), (GOLD, 0), (M64, 0), (1, (3 << 32) | EPS),
              (0, M64), (EPS, (1 << 32) | 1)]
    rng = random.Random(0x63)
    pairs += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(3000)]
    return interleave(pairs)


def add_mul_eps_pairs():
    words = GL_VALUES + [M64, M64 - 1, GOLD, GOLD + 1]
    hs = [0, 1, 2, EPS, EPS - 1, 1 << 31, (1 << 31) - 1, 1 << 16]
    pairs = [(a, h) for a in words for h in hs]
    rng = random.Random(0x64)
    pairs += [(rng.getrandbits(64), rng.getrandbits(32)) for _ in range(3000)]
    return interleave(pairs)


def u64(vals):
    return np.array(vals, dtype=np.uint64)


# ---- register DFT blocks ------------------------------------------------------------------------
def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def w64(e64):
    """w_64 = 2^E64: 2^39 forward, 2^153 its inverse (ntt_gl.hpp header)."""
    return pow(2, e64, GOLD)


def dft_rows():
    """16-value rows: the unit impulses (every output is then one signed power of two), all
    p - 1, draws from the edge values, random rows."""
    rows = [[1 if i == j else 0 for i in range(16)] for j in range(16)]
    rows += [[GOLD - 1 if i == j else 0 for i in range(16)] for j in range(16)]
    rows.append([GOLD - 1] * 16)
    rows.append([1] * 16)
    rng = random.Random(0x65)
    rows += [[rng.choice(GL_VALUES) for _ in range(16)] for _ in range(150)]
    rows += [[rng.randrange(GOLD) for _ in range(16)] for _ in range(150)]
    return interleave(rows)


def ref_dft(row, logq, w):
    """Independent 2^logq-point DFTs over consecutive groups of the row, X_k = sum_j x_j w^(jk),
    natural order in, output k at position bitrev(k) of its group."""
    q = 1 << logq
    out = [0] * len(row)
    pw = [pow(w, e, GOLD) for e in range(q)]
    for g in range(0, len(row), q):
        for k in range(q):
            out[g + bitrev(k, logq)] = sum(row[g + j] * pw[(j * k) % q] for j in range(q)) % GOLD
    return out


def ref_stage_b(row, e64, q1):
    """Stage B of one q1 (ntt_gl.hpp header): Z[s2] *= w_64^(s2 q1), then the 16-point DFT over
    s2 with w_16 = w_64^4; output q2 at position bitrev4(q2)."""
    w = w64(e64)
    tw = [row[s2] * pow(w, s2 * q1, GOLD) % GOLD for s2 in range(16)]
    return ref_dft(tw, 4, pow(w, 4, GOLD))


def ref_post_twiddle_br(row, e64, q):
    w = w64(e64)
    out = list(row)
    for e in range(16):
        out[bitrev(e, 4)] = row[bitrev(e, 4)] * pow(w, e * q, GOLD) % GOLD
    return out


def ref_rg3_c_shift(row, e64, wv):
    w = w64(e64)
    out = list(row)
    for u in range(4):
        for r2 in range(4):
            out[u * 4 + r2] = row[u * 4 + r2] * pow(w, r2 * (wv + 4 * u), GOLD) % GOLD
    return out


# ---- Mod32 --------------------------------------------------------------------------------------
def mod32_pairs(m, n=1500):
    edge = sorted({0, 1 % m, m - 1, (m - 2) % m})
    pairs = [(a, b) for a in edge for b in edge]
    rng = random.Random(m)
    pairs += [(rng.randrange(m), rng.randrange(m)) for _ in range(n)]
    return interleave(pairs)


def barrett_corrections(a, b, m):
    """How many of Mod32::mul's conditional subtractions a b takes (mu = floor(2^64 / m))."""
    x = a * b
    r = x - ((x * ((1 << 64) // m)) >> 64) * m
    return r // m


# ---- 256-bit fields -----------------------------------------------------------------------------
def fp_values(p):
    """0, 1, 2, p - 1, p - 2, (p +- 1) / 2, and for each limb boundary k a run of all-ones limbs
    below it, a run of zero limbs below it, and ones / zeros runs that start at limb 1."""
    v = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    for k in range(1, 8):
        v += [(1 << (32 * k)) - 1, 1 << (32 * k), (1 << (32 * k)) - (1 << 32), (1 << (32 * k)) + 1]
    top = (p >> 224) << 224  # boundary 8 is the top of the number: the largest runs below p
    v += [top - 1, top, top - (1 << 32)]
    assert all(0 <= x < p for x in v)
    return sorted(set(v))


def fp_random(p, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(p) for _ in range(n)]


def fp_pairs_chosen(p):
    ev = fp_values(p)
    pairs = [(a, b) for a in ev for b in ev]
    some = ev + fp_random(p, 40, 0x70)
    for a in some:
        for s in (p - 1, p, p + 1):  # a + b on both sides of the final select, and on it
            b = s - a
            if 0 <= b < p:
                pairs.append((a, b))
        pairs.append((a, a))
        if a + 1 < p:
            pairs.append((a, a + 1))  # a = b - 1: the subtraction borrows through every limb
    return pairs


def fp_pairs_random(p, n=1200, seed=0x71):
    v = fp_random(p, 2 * n, seed)
    return list(zip(v[:n], v[n:]))


def fp_pairs(p):
    return interleave(fp_pairs_chosen(p) + fp_pairs_random(p))


def fp_reduce_inputs(p):
    """Inputs of reduce_once, below 2 p: the values, and the values plus p."""
    v = fp_values(p) + fp_random(p, 600, 0x72)
    return interleave(v + [x + p for x in v])


def wide_values(p, n=700, seed=0x73, bound=R256):
    """Integers below `bound` (default: any 256-bit word) for the lazily reduced 29-bit-limb
    code: the field's edge values, multiples of p and their neighbours, all-ones runs up to the
    top limb, random words."""
    v = fp_values(p) + [k * p + d for k in range(1, 6) for d in (-1, 0, 1)]
    v += [R256 - 1, R256 - 2, R256 - (1 << 32), 1 << 255, (1 << 255) - 1, R256 - (1 << 224), (1 << 232) - 1, 1 << 232]
    v += [((1 << 29 * k) - 1) for k in range(1, 9)] + [1 << 29 * k for k in range(1, 9)]  # 29-bit limb boundaries
    rng = random.Random(seed)
    v += [rng.getrandbits(256) for _ in range(n)]
    return interleave([x % bound for x in v], seed)


def wide_pairs(p, seed=0x74, bound=R256):
    a = wide_values(p, seed=seed, bound=bound)
    b = wide_values(p, seed=seed + 1, bound=bound)
    return list(zip(a, b))


def lazy_pairs(p, m, bound, seed):
    """(x0, x1), 256-bit words whose lazy difference x0 + m p - x1 (what l29::sub(x0, x1, M) holds,
    M = m p) stays below `bound`: the wide pairs where they already do (differences of either
    sign), the others pulled in as x1 + d, d < bound - m p, and the bound itself (bound - 1)."""
    lim = bound - m * p
    assert 0 < lim < R256
    out = []
    for u, v in wide_pairs(p, seed=seed):
        if u - v >= lim:
            v %= R256 - lim
            u = v + u % lim
        out.append((u, v))
    out += [(v + lim - 1, v) for v in (0, 1, p, R256 - lim) if v + lim <= R256]
    assert all(0 <= u < R256 and 0 <= v < R256 and 0 < u + m * p - v < bound for u, v in out)
    return interleave(out, seed)


def limbs29(x):
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]


def mont_unreduced(a, b, p):
    """(a b + m p) / 2^256 with m = -a b p^-1 mod 2^256: what the column scan holds before its
    reduce_once (below 2 p); the final select takes t - p when t >= p."""
    t = a * b
    m = (t * (R256 - pow(p, -1, R256))) % R256
    assert (t + m * p) % R256 == 0
    return (t + m * p) >> 256


def fp_add_model(a, b, p, wrong=False):
    """256-bit add by its select. wrong: the select taken with > instead of >= (a deliberately
    wrong model, tests/test_field_device_inputs.py)."""
    s = a + b
    return s - p if (s > p if wrong else s >= p) else s


def u256(vals):
    """ints -> (n, 4) uint64, little-endian limbs (the ABI layout)."""
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), 4).copy()


def from_u256(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
