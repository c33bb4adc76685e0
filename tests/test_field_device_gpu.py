"""The device paths of the field headers, function by function, against Python integers.

The code that runs on the GPU is not the code a host build of the headers runs: Goldilocks
sub / reduce128 / add_mul_eps (csrc/field.hpp) and the 256-bit add / sub / reduce_once / mul*
(csrc/fp256.hpp) are inline-assembly carry chains on the device, the 29-bit-limb code
(csrc/fr29.hpp, csrc/msm_l29.hpp) and Mod32 are device-only, and the register DFT blocks of
csrc/ntt_kernels.hpp / ntt_gl.hpp exist only inside the pass kernels. tests/native/
field_device_check.hip (built by __graft_entry__.build() into tests/native/
libfield_device_check.so) calls each of them in a one-thread-per-element kernel; here every
result is compared bit for bit with integer arithmetic, on operands chosen so that every
correction of every reduction is taken (tests/field_device_inputs.py; the conditions are
asserted before the GPU is called, and tests/test_field_device_inputs.py shows on the CPU that a
wrong correction would be seen). Operand arrays are in a fixed shuffled order and their length
is no multiple of 64: the carries are per-lane masks, and the last wave is partial.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import field_device_inputs as fdi  # noqa: E402
from field_device_inputs import EPS, FQ, FR, GOLD, M64, R256, R261  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(HERE, "native", "libfield_device_check.so")

# op codes of field_device_check.hip
(GL_ADD, GL_SUB, GL_MUL, GL_REDUCE128, GL_ADD_MUL_EPS, GL_MUL_POW2, GL_DIV_POW2, GL_POW2, GL_POW2_ABS) = range(9)
(DFT_REG, DFT_REG_TABLE, DFT_STAGE_B, DFT_POST_TWIDDLE_BR, DFT_RG3_C_SHIFT) = range(10, 15)
(M32_ADD, M32_SUB, M32_MUL) = range(20, 23)
(FP_ADD, FP_SUB, FP_REDUCE_ONCE, FP_MUL, FP_MUL_TP, FP_MUL2, FP_MULN3, FP_MULN4, FP_TO_MONT, FP_FROM_MONT) = range(30, 40)
(FR29_MUL, FR29_ADD, FR29_SUB) = range(50, 53)
(L29_RELIMB, L29_MUL, L29_SQR, L29_MULSUB, L29_MUL_SHIFT_SUB, L29_NORM, L29_SUB, L29_CANON, L29_ZERO_MOD_P,
 L29_TIMES32) = range(60, 70)
MAX_COUNT = 1 << 16


class Harness:
    def __init__(self):
        assert os.path.exists(LIB), "tests/native/libfield_device_check.so missing: run __graft_entry__.build()"
        self.lib = ctypes.CDLL(LIB)
        vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
        self.lib.fdc_run.restype = ctypes.c_int
        self.lib.fdc_run.argtypes = [ctypes.c_int, u64, u64, vp, vp, vp, sz]
        self.lib.fdc_layout.restype = ctypes.c_int
        self.lib.fdc_layout.argtypes = [ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int)]

    def run(self, op, a, b=None, p0=0, p1=0):
        """a, b: uint64 arrays of count x (words per element); returns count x (words per output)."""
        lay = (ctypes.c_int * 4)()
        assert self.lib.fdc_layout(op, p0, p1, lay) == 0, "unknown op %d or parameter (%d, %d)" % (op, p0, p1)
        aw, bw, ow, bsh = lay
        a = np.ascontiguousarray(a, dtype=np.uint64)
        assert a.size % aw == 0
        count = a.size // aw
        assert 0 < count <= MAX_COUNT and count % 64 != 0
        if bw:
            b = np.ascontiguousarray(b, dtype=np.uint64)
            assert b.size == (bsh if bsh else count * bw)
        out = np.empty(count * ow, dtype=np.uint64)
        rc = self.lib.fdc_run(op, p0, p1, a.ctypes.data, b.ctypes.data if bw else None, out.ctypes.data, count)
        if rc != 0:  # a HIP error is sticky for the process: nothing more may run on the device
            pytest.exit("fdc_run(op %d, %d, %d) returned HIP error %d" % (op, p0, p1, rc), returncode=3)
        return out.reshape(count, ow) if ow > 1 else out


@pytest.fixture(scope="module")
def fdc():
    return Harness()


def same(got, ref, what=""):
    got = [int(x) for x in np.asarray(got).reshape(-1)]
    ref = [int(x) for x in ref]
    assert len(got) == len(ref)
    bad = [i for i in range(len(ref)) if got[i] != ref[i]]
    assert not bad, "%s: %d of %d differ, first at %d: got %#x, expected %#x" % (
        what, len(bad), len(ref), bad[0], got[bad[0]], ref[bad[0]])


def same256(got, ref, what=""):
    got = fdi.from_u256(got)
    assert len(got) == len(ref)
    bad = [i for i in range(len(ref)) if got[i] != ref[i]]
    assert not bad, "%s: %d of %d differ, first at %d: got %#x, expected %#x" % (
        what, len(bad), len(ref), bad[0], got[bad[0]], ref[bad[0]])


# ---- Goldilocks -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gl_pairs():
    return fdi.gl_pairs()


@pytest.fixture(scope="module")
def gl_unary():
    return fdi.gl_unary()


def test_gl_mul(fdc, gl_pairs):
    cases = fdi.count_cases((fdi.red96_case(*fdi.mul_red96_args(a, b)) for a, b in gl_pairs), fdi.RED96_CASES)
    print("gl mul reduction cases:", cases)
    assert all(cases[c] >= 3 for c in fdi.RED96_CASES), cases
    low = fdi.low_word_counts(fdi.mul_red96_args(a, b) for a, b in gl_pairs)
    print("gl mul low-word borrow / carry of the correction:", low)
    assert low["c3"] >= 3 and low["c4"] >= 3, low
    a, b = zip(*gl_pairs)
    same(fdc.run(GL_MUL, fdi.u64(a), fdi.u64(b)), [x * y % GOLD for x, y in gl_pairs], "mul")


def test_gl_add_sub(fdc, gl_pairs):
    # both outcomes of add's correction (wrap; no wrap and s >= p) and of sub's (borrow; and the
    # correction's own borrow out of the low word, lo = 0xFFFFFFFF.. patterns)
    assert sum(a + b > M64 for a, b in gl_pairs) >= 3 and sum(GOLD <= a + b <= M64 for a, b in gl_pairs) >= 3
    assert sum(a < b for a, b in gl_pairs) >= 3 and sum(a < b and (a - b) & EPS == EPS for a, b in gl_pairs) >= 3
    a, b = zip(*gl_pairs)
    same(fdc.run(GL_ADD, fdi.u64(a), fdi.u64(b)), [(x + y) % GOLD for x, y in gl_pairs], "add")
    same(fdc.run(GL_SUB, fdi.u64(a), fdi.u64(b)), [(x - y) % GOLD for x, y in gl_pairs], "sub")


def test_gl_reduce128(fdc):
    pairs = fdi.reduce128_pairs()
    cases = fdi.count_cases((fdi.red96_case(lo, hi & EPS, hi >> 32) for lo, hi in pairs), fdi.RED96_CASES)
    print("gl reduce128 cases:", cases)
    assert all(cases[c] >= 3 for c in fdi.RED96_CASES), cases
    low = fdi.low_word_counts((lo, hi & EPS, hi >> 32) for lo, hi in pairs)
    print("gl reduce128 low-word borrow / carry of the correction:", low)
    assert low["c3"] >= 3 and low["c4"] >= 3, low
    lo, hi = zip(*pairs)
    same(fdc.run(GL_REDUCE128, fdi.u64(lo), fdi.u64(hi)), [(x + (y << 64)) % GOLD for x, y in pairs], "reduce128")


def test_gl_add_mul_eps(fdc):
    pairs = fdi.add_mul_eps_pairs()
    cases = fdi.count_cases((fdi.addmul_eps_case(lo, h) for lo, h in pairs), fdi.ADDMUL_CASES)
    print("gl add_mul_eps cases:", cases)
    assert all(cases[c] >= 3 for c in fdi.ADDMUL_CASES), cases
    lo, h = zip(*pairs)
    same(fdc.run(GL_ADD_MUL_EPS, fdi.u64(lo), fdi.u64(h)), [(x + y * EPS) % GOLD for x, y in pairs], "add_mul_eps")


@pytest.mark.parametrize("lo,hi", [(0, 33), (33, 64), (64, 96)])
def test_gl_mul_pow2(fdc, gl_unary, lo, hi):
    for s in range(max(lo, 33), min(hi, 64)):  # the shifts that go through gl_red96
        got = fdi.count_cases((fdi.red96_case(*fdi.mul_pow2_red96_args(x, s)) for x in gl_unary), fdi.RED96_CASES)
        assert tuple(c for c in fdi.RED96_CASES if got[c]) == fdi.MUL_POW2_REACH[s], (s, got)
        if s in (33, 48, 63):
            print("gl mul_pow2<%d> reduction cases:" % s, got)
    if lo == 33:  # over all these shifts: the correction's low-word borrow (x = 2^(97-S) - 1) and carry
        low = fdi.low_word_counts(fdi.mul_pow2_red96_args(x, s) for s in range(33, 64) for x in gl_unary)
        print("gl mul_pow2 low-word borrow / carry of the correction:", low)
        assert low["c3"] >= 3 and low["c4"] >= 3, low
    x = fdi.u64(gl_unary)
    for s in range(lo, hi):
        same(fdc.run(GL_MUL_POW2, x, p0=s), [(v << s) % GOLD for v in gl_unary], "mul_pow2<%d>" % s)


def test_gl_div_pow2(fdc, gl_unary):
    x = fdi.u64(gl_unary)
    for k in range(1, 33):
        inv = pow(2, -k, GOLD)
        same(fdc.run(GL_DIV_POW2, x, p0=k), [v * inv % GOLD for v in gl_unary], "gl_div_pow2<%d>" % k)


@pytest.mark.parametrize("lo", [0, 64, 128])
def test_gl_pow2(fdc, gl_unary, lo):
    x = fdi.u64(gl_unary)
    for k in range(lo, lo + 64):
        w = pow(2, k, GOLD)
        ref = [v * w % GOLD for v in gl_unary]
        same(fdc.run(GL_POW2, x, p0=k), ref, "gl_pow2<%d>" % k)
        got = fdc.run(GL_POW2_ABS, x, p0=k)
        neg = int(got[0, 1])
        assert neg in (0, 1) and all(int(n) == neg for n in got[:, 1])
        same(got[:, 0], [(GOLD - r) % GOLD for r in ref] if neg else ref, "gl_pow2_abs<%d>, gl_pow2_neg %d" % (k, neg))


# ---- register DFT blocks --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    return fdi.dft_rows()


def flat(rows_):
    return fdi.u64([x for r in rows_ for x in r])


@pytest.mark.parametrize("e64", [39, 153])
@pytest.mark.parametrize("logq", [1, 2, 3, 4])
def test_dft_reg(fdc, rows, logq, e64):
    w = pow(fdi.w64(e64), 64 >> logq, GOLD)
    assert pow(w, 1 << logq, GOLD) == 1 and pow(w, 1 << (logq - 1), GOLD) == GOLD - 1
    same(fdc.run(DFT_REG, flat(rows), p0=logq, p1=e64), [x for r in rows for x in fdi.ref_dft(r, logq, w)])


def test_dft_reg_table_twiddles(fdc, rows):
    w = pow(7, 3 * (GOLD - 1) // 16, GOLD)  # a primitive 16th root, from the table as general factors
    assert pow(w, 8, GOLD) == GOLD - 1
    wq = fdi.u64([pow(w, m, GOLD) for m in range(8)])
    same(fdc.run(DFT_REG_TABLE, flat(rows), wq), [x for r in rows for x in fdi.ref_dft(r, 4, w)])


@pytest.mark.parametrize("e64", [39, 153])
@pytest.mark.parametrize("q1", [0, 1, 2, 3])
def test_stage_b(fdc, rows, q1, e64):
    """gl_stage_b_head<E64, Q1> then dft_reg_tail: the twiddle without its signs, the signed
    first levels (dft_reg_signed with gl_stage_b_negmask(E64, Q1)), the common last levels."""
    same(fdc.run(DFT_STAGE_B, flat(rows), p0=e64, p1=q1), [x for r in rows for x in fdi.ref_stage_b(r, e64, q1)])


@pytest.mark.parametrize("e64", [39, 153])
@pytest.mark.parametrize("q", [1, 2, 3])
def test_post_twiddle_br(fdc, rows, q, e64):
    same(fdc.run(DFT_POST_TWIDDLE_BR, flat(rows), p0=e64, p1=q),
         [x for r in rows for x in fdi.ref_post_twiddle_br(r, e64, q)])


@pytest.mark.parametrize("e64", [39, 153])
@pytest.mark.parametrize("wv", [0, 1, 2, 3])
def test_rg3_c_shift(fdc, rows, wv, e64):
    same(fdc.run(DFT_RG3_C_SHIFT, flat(rows), p0=e64, p1=wv), [x for r in rows for x in fdi.ref_rg3_c_shift(r, e64, wv)])


# ---- Mod32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", fdi.MOD32_MODULI)
def test_mod32(fdc, m):
    pairs = fdi.mod32_pairs(m)
    if m in (3221225473, (1 << 32) - 5, (1 << 31) + 11):
        assert any(fdi.barrett_corrections(a, b, m) == 1 for a, b in pairs)
    a, b = (fdi.u64(v) for v in zip(*pairs))
    mu = (1 << 64) // m
    same(fdc.run(M32_ADD, a, b, p0=m, p1=mu), [(x + y) % m for x, y in pairs], "add mod %d" % m)
    same(fdc.run(M32_SUB, a, b, p0=m, p1=mu), [(x - y) % m for x, y in pairs], "sub mod %d" % m)
    same(fdc.run(M32_MUL, a, b, p0=m, p1=mu), [x * y % m for x, y in pairs], "mul mod %d" % m)


# ---- Fp256 ------------------------------------------------------------------------------------------
FIELDS = [pytest.param(0, FR, id="Fr"), pytest.param(1, FQ, id="Fq")]


def both_sides(taken, what):
    n = sum(1 for t in taken if t)
    assert min(n, len(taken) - n) >= 16, "%s: the final select goes one way only (%d of %d)" % (what, n, len(taken))


@pytest.mark.parametrize("fid,p", FIELDS)
def test_fp256_add_sub_reduce_once(fdc, fid, p):
    pairs = fdi.fp_pairs(p)
    red = fdi.fp_reduce_inputs(p)
    both_sides([a + b >= p for a, b in pairs], "add")
    both_sides([a < b for a, b in pairs], "sub")
    both_sides([x >= p for x in red], "reduce_once")
    assert {a + b for a, b in pairs} >= {p - 1, p, p + 1} and max(red) == 2 * p - 1
    a, b = (fdi.u256(v) for v in zip(*pairs))
    same256(fdc.run(FP_ADD, a, b, p0=fid), [(x + y) % p for x, y in pairs], "add")
    same256(fdc.run(FP_SUB, a, b, p0=fid), [(x - y) % p for x, y in pairs], "sub")
    same256(fdc.run(FP_REDUCE_ONCE, fdi.u256(red), p0=fid), [x % p for x in red], "reduce_once")


@pytest.mark.parametrize("fid,p", FIELDS)
def test_fp256_mul(fdc, fid, p):
    """mul, mul_tp, mul2, mulN<3>, mulN<4> (separate outputs, and outputs aliasing the inputs),
    to_mont, from_mont: all the Montgomery product a b 2^-256."""
    pairs = fdi.fp_pairs(p)
    both_sides([fdi.mont_unreduced(a, b, p) >= p for a, b in pairs], "mul")
    rinv = pow(R256, -1, p)
    ref = [x * y * rinv % p for x, y in pairs]
    n = len(pairs)
    a, b = (fdi.u256(v) for v in zip(*pairs))
    same256(fdc.run(FP_MUL, a, b, p0=fid), ref, "mul")
    same256(fdc.run(FP_MUL_TP, a, b, p0=fid), ref, "mul_tp")
    same256(fdc.run(FP_MUL2, a, b, p0=fid), [ref[(i + j) % n] for i in range(n) for j in range(2)], "mul2")
    for op, k in ((FP_MULN3, 3), (FP_MULN4, 4)):
        for alias in (0, 1):
            same256(fdc.run(op, a, b, p0=fid, p1=alias), [ref[(i + j) % n] for i in range(n) for j in range(k)],
                    "mulN<%d>, alias %d" % (k, alias))
    xs = [x for x, _ in pairs]
    same256(fdc.run(FP_TO_MONT, a, p0=fid), [x * R256 % p for x in xs], "to_mont")
    same256(fdc.run(FP_FROM_MONT, a, p0=fid), [x * rinv % p for x in xs], "from_mont")


# ---- fr29: lazily reduced 29-bit limbs of Fr ------------------------------------------------------
def two(pairs):
    return fdi.u256([x for pr in pairs for x in pr])


def test_fr29(fdc):
    """Operands as the radix-4 stage of ntt256l_pass_kernel forms them (field_device_check.hip
    Fr29*): sums of canonical values (below 2 r, limbs below 2^30), a product's output (below
    2 r), reduce()'s output (below 2 r + 2^234); every result leaves through reduce and canon."""
    pa = fdi.fp_pairs(FR)
    pb = fdi.interleave(pa, seed=0x29)[:len(pa)]
    assert len(pa) == len(pb)
    # the lazy ranges are entered: sums above r on both sides
    assert sum(a0 + a1 >= FR for a0, a1 in pa) >= 16 and sum(b0 + b1 >= FR for b0, b1 in pb) >= 16
    rinv = pow(R261, -1, FR)
    a, b = two(pa), two(pb)
    same256(fdc.run(FR29_MUL, a, b), [x[0] * y[0] * rinv % FR for x, y in zip(pa, pb)], "mul")
    same256(fdc.run(FR29_ADD, a, b), [(sum(x) + sum(y)) % FR for x, y in zip(pa, pb)], "add")
    same256(fdc.run(FR29_SUB, a, b, p0=2), [(sum(x) - y[0] * y[1] * rinv) % FR for x, y in zip(pa, pb)], "sub B2R")
    same256(fdc.run(FR29_SUB, a, b, p0=4), [(sum(x) - sum(y)) % FR for x, y in zip(pa, pb)], "sub B4R")
    same256(fdc.run(FR29_SUB, a, b, p0=8), [(sum(x) - 3 * y[0] - y[1]) % FR for x, y in zip(pa, pb)], "sub B8R")


# ---- l29: lazily reduced 29-bit limbs of Fq (the MSM accumulation) -----------------------------------
def lazy_val(pr, m):
    """What the harness's lazy<M>(x0, x1) holds: x0 (M = 0) or x0 + M p - x1."""
    return pr[0] if m == 0 else pr[0] + m * FQ - pr[1]


@pytest.mark.parametrize("m", [0, 8, 16])
def test_l29_mul_sqr(fdc, m):
    """mul and sqr at the bound msm_l29.hpp states for a product's inputs, normalised values below
    17.3 p: operands formed on the device as l29::sub(x0, x1, M16P) = x0 + 16 p - x1 and kept
    below 17.3 p here (M = 8: around 8 p; M = 0: any 256-bit word)."""
    rinv = pow(R261, -1, FQ)
    bound = 173 * FQ // 10
    if m == 0:
        pa, pb = fdi.wide_pairs(FQ), fdi.wide_pairs(FQ, seed=0x84)
        assert max(x for x, _ in pa) == R256 - 1
    else:
        pa, pb = (fdi.lazy_pairs(FQ, m, bound if m == 16 else (m + 5) * FQ, seed) for seed in (0x85 + m, 0x95 + m))
    va, vb = [lazy_val(x, m) for x in pa], [lazy_val(x, m) for x in pb]
    assert max(va + vb) < bound
    if m == 16:  # the bound is reached, and so is the low side of the lazy range
        assert max(va) == bound - 1 and max(vb) == bound - 1 and min(va) < 12 * FQ
        assert sum(x >= 17 * FQ for x in va) >= 16
    same256(fdc.run(L29_MUL, two(pa), two(pb), p0=m), [x * y * rinv * 32 % FQ for x, y in zip(va, vb)], "mul")
    same256(fdc.run(L29_SQR, two(pa), p0=m), [x * x * rinv * 32 % FQ for x in va], "sqr")


def test_l29_mulsub_mul_shift_sub(fdc):
    """mulsub and mul_shift_sub with operands as madd gives them, at the stated bounds: mulsub's
    a, b below 17.3 p, c (Y) below 11.3 p, d (PPP) below 3.3 p; mul_shift_sub's f below 11.3 p
    with E = 12 p (X) and below 3.8 p with E = 4 p (Y); and both on plain 256-bit words."""
    rinv = pow(R261, -1, FQ)
    b173, b113, b33, b38 = 173 * FQ // 10, 113 * FQ // 10, 33 * FQ // 10, 38 * FQ // 10
    pa, pb = fdi.lazy_pairs(FQ, 16, b173, 0xA1), fdi.lazy_pairs(FQ, 16, b173, 0xA2)
    pc = fdi.lazy_pairs(FQ, 8, b113, 0xA3)
    n = len(pa)
    assert len(pb) == n and len(pc) == n
    wd = fdi.wide_values(FQ, seed=0xA4)
    d = [b33 - 1 if i % 97 == 0 else wd[i % len(wd)] % b33 for i in range(n)]
    va, vb, vc = ([lazy_val(x, k) for x in ps] for ps, k in ((pa, 16), (pb, 16), (pc, 8)))
    assert max(va) == b173 - 1 and max(vb) == b173 - 1 and max(vc) == b113 - 1 and max(d) == b33 - 1
    assert sum(x >= 11 * FQ for x in vc) >= 16 and min(vc) < 4 * FQ
    # the largest c d together, and the largest a b: the signed columns at both ends
    assert max(x * y for x, y in zip(vc, d)) > 30 * FQ * FQ and max(x * y for x, y in zip(va, vb)) > 280 * FQ * FQ
    a4 = fdi.u256([x for i in range(n) for x in pa[i] + pb[i]])
    b4 = fdi.u256([x for i in range(n) for x in pc[i] + (d[i], 0)])
    same256(fdc.run(L29_MULSUB, a4, b4, p0=1),
            [(va[i] * vb[i] - vc[i] * d[i]) * rinv * 32 % FQ for i in range(n)], "mulsub at its bounds")
    same256(fdc.run(L29_MULSUB, a4, b4, p0=0),
            [(pa[i][0] * pb[i][0] - pc[i][0] * d[i]) * rinv * 32 % FQ for i in range(n)], "mulsub, 256-bit words")
    # mul_shift_sub: x, y any 256-bit words (the point coordinate and ZZ / ZZZ are below 3.3 p)
    wp = fdi.wide_pairs(FQ, seed=0xA5)
    xy = [wp[i % len(wp)] for i in range(n)]
    ref = lambda f: [(x[0] * x[1] * rinv - fi) * 32 % FQ for x, fi in zip(xy, f)]  # noqa: E731
    assert sum(x >= 11 * FQ for x in vc) >= 16
    same256(fdc.run(L29_MUL_SHIFT_SUB, two(xy), two(pc), p0=12, p1=1), ref(vc), "mul_shift_sub 12 p, f to 11.3 p")
    f12 = [x for x, _ in pc]
    same256(fdc.run(L29_MUL_SHIFT_SUB, two(xy), two(pc), p0=12, p1=0), ref(f12), "mul_shift_sub 12 p, f a word")
    f4 = [b38 - 1 if i % 89 == 0 else x % b38 for i, x in enumerate(f12)]
    assert max(f4) == b38 - 1 and sum(f >= 3 * FQ for f in f4) >= 16
    same256(fdc.run(L29_MUL_SHIFT_SUB, two(xy), two([(f, 0) for f in f4]), p0=4), ref(f4), "mul_shift_sub 4 p")


def test_l29_linear(fdc):
    """norm, sub (8 p and 16 p), canon, zero_mod_p, times32 at the bounds their comments state."""
    pw = fdi.wide_pairs(FQ, seed=0x94)
    a, b = (fdi.u256(v) for v in zip(*pw))
    assert max(x for x, _ in pw) == R256 - 1
    same256(fdc.run(L29_RELIMB, a), [x for x, _ in pw], "from_u256 / to_u256")
    same256(fdc.run(L29_SUB, a, b, p0=8), [(x - y) * 32 % FQ for x, y in pw], "sub 8 p")
    same256(fdc.run(L29_SUB, a, b, p0=16), [(x - y) * 32 % FQ for x, y in pw], "sub 16 p")
    # norm at its bound (limbs below 2^32): M16P's redundant limbs (up to 0x985d977d) plus three
    # values' limbs; the all-ones words give every low limb its largest sum, M16P[i] + 0x5ffffffd
    x2 = [y for _, y in fdi.wide_pairs(FQ, seed=0x96)]
    trip = [(R256 - 1,) * 3, (R256 - 1, 0, R256 - 1), (0, 0, 0)] + [(x, y, z) for (x, y), z in zip(pw, x2)]
    trip = trip[:len(pw)]
    assert all(sum(fdi.limbs29(v)[i] for v in trip[0]) == 3 * ((1 << 29) - 1) for i in range(8))
    same256(fdc.run(L29_NORM, two([t[:2] for t in trip]), fdi.u256([t[2] for t in trip])),
            [sum(t) * 32 % FQ for t in trip], "norm")
    below2p = fdi.fp_reduce_inputs(FQ)
    assert 0 in below2p and FQ in below2p and FQ - 1 in below2p and FQ + 1 in below2p and 2 * FQ - 1 in below2p
    same256(fdc.run(L29_CANON, fdi.u256(below2p)), [x % FQ for x in below2p], "canon")
    same(fdc.run(L29_ZERO_MOD_P, fdi.u256(below2p)), [int(x % FQ == 0) for x in below2p], "zero_mod_p")
    canon = fdi.interleave(fdi.fp_values(FQ) + fdi.fp_random(FQ, 800, 0x95))
    same256(fdc.run(L29_TIMES32, fdi.u256(canon)), [32 * x % FQ for x in canon], "times32")
