"""The BN254 G1 group law on the device, exit by exit, against the group and against the formulas.

Every point addition of csrc/ec_bn254.hpp (G1::madd, madd_tp, add, add2 / dbl2, G1Quad::add /
dbl) and of csrc/msm_l29.hpp (l29::madd with its callers' reload-and-double, the raw accumulator
round trip store_raw / raw_to_xyzz) has four exits: an identity operand, P + P, P + (-P), the
generic formula. tests/native/group_device_check.hip (built by __graft_entry__.build() into
tests/native/libgroup_device_check.so) calls each function in a one-thread-per-element kernel
(one quad per element for G1Quad) on the operands of tests/group_device_inputs.py, which enter
every exit, also with the two operands in different XYZZ representations of one point -- the
only case in which U1 == U2 is a cross-multiplied comparison and not a copy. Each result is
checked twice: against the group (the oracle's g1_add / g1_mul on the discrete logs) and,
coordinate for coordinate, against the integer restatement of the EFD formula with the exits
the code states. The case counts are asserted before the GPU is called
(tests/test_group_device_inputs.py shows on the CPU that a wrong exit would be seen). Operand
arrays are in a fixed shuffled order and their length is no multiple of 64.

Exits entered, by test (the MSM kernels' share is in tests/test_msm_gpu.py):
  G1::add, add2, G1Quad::add   p identity, q identity, both (G1::identity() and ZZ = 0 with any
                               X, Y), P + P -> dbl / dbl2 / G1Quad::dbl (same and different
                               representations), P + (-P) -> identity(), generic: test_add,
                               test_quad_add (adjacent quads of a wave on different exits)
  G1::madd, madd_tp            p identity -> from_affine, P + P -> mdbl(a), P + (-P), generic,
                               the affine operand equal / opposite to a non-trivial
                               representation: test_madd
  G1::dbl, dbl2, G1Quad::dbl   identity returned as it is, generic: test_dbl; G1::mdbl: no exit
  G1::mul_small                k = 0 (no bit: identity), k = 1, powers of two (dbl only), odd k,
                               2^32 - 1, and the identity as the point: test_mul_small
  G1::to_affine_plain, inv     identity -> (0, 0), generic: test_to_affine_plain
  l29::to_xyzz, store_raw,     id = false and id = true over live coordinates:
  raw_to_xyzz, from_xyzz       test_accumulator_round_trip, test_accumulation_chain
  l29::madd + its callers      id -> start_run, P == 0 and R == 0 (true: reload, mdbl) with an
                               affine-like and a projective accumulator, P == 0 and R != 0 (id),
                               generic; first, middle and last step: test_accumulation_chain
Not reachable through the harness: which of its two accepted values (0 or p) zero_mod_p sees in
l29::madd is decided by the lazy reduction, not by the operands (the field harness tests both
directly); G1::inv(0), from_xyzz of the identity and an affine identity operand of madd are outside
the functions' contracts (the MSM filters such points before the accumulation).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import group_device_inputs as gdi  # noqa: E402
from group_device_inputs import IDENTITY, Q  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(HERE, "native", "libgroup_device_check.so")

# op codes of group_device_check.hip
(G_MDBL, G_DBL, G_DBL2, G_MADD, G_MADD_TP, G_ADD, G_ADD2, G_MUL_SMALL, G_TO_AFFINE) = range(9)
(Q_ADD, Q_DBL) = range(20, 22)
(ACC_XYZZ, ACC_RAW, ACC_CHAIN, G_CHAIN) = range(30, 34)
MAX_COUNT = 1 << 14


class Harness:
    def __init__(self):
        assert os.path.exists(LIB), "tests/native/libgroup_device_check.so missing: run __graft_entry__.build()"
        self.lib = ctypes.CDLL(LIB)
        vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
        self.lib.gdc_run.restype = ctypes.c_int
        self.lib.gdc_run.argtypes = [ctypes.c_int, u64, u64, vp, vp, vp, sz]
        self.lib.gdc_layout.restype = ctypes.c_int
        self.lib.gdc_layout.argtypes = [ctypes.c_int, u64, u64, ctypes.POINTER(ctypes.c_int)]

    def run(self, op, a, b=None, p0=0):
        """a, b: lists of tuples of plain integers (one tuple per element); returns the output
        words as a (count, words) uint64 array."""
        lay = (ctypes.c_int * 4)()
        assert self.lib.gdc_layout(op, p0, 0, lay) == 0, "unknown op %d or parameter %d" % (op, p0)
        aw, bw, ow, _ = lay
        count = len(a)
        assert 0 < count <= MAX_COUNT and count % 64 != 0
        a = np.ascontiguousarray(gdi.pack(a))
        assert a.size == count * aw
        if bw:
            assert len(b) == count
            b = np.ascontiguousarray(gdi.pack(b))
            assert b.size == count * bw
        out = np.empty(count * ow, dtype=np.uint64)
        rc = self.lib.gdc_run(op, p0, 0, a.ctypes.data, b.ctypes.data if bw else None, out.ctypes.data, count)
        if rc != 0:  # a HIP error is sticky for the process: nothing more may run on the device
            pytest.exit("gdc_run(op %d, %d) returned HIP error %d" % (op, p0, rc), returncode=3)
        return out.reshape(count, ow)

    def points(self, op, a, b=None, p0=0):
        """The outputs as one XYZZ tuple per element."""
        return gdi.unpack(self.run(op, a, b, p0), 4)


@pytest.fixture(scope="module")
def gdc():
    return Harness()


def both_checks(got, want_pts, model, what):
    """got: device XYZZ tuples; want_pts: the group's affine points (None: the identity); model:
    the formula restatement's XYZZ tuples."""
    assert len(got) == len(want_pts) == len(model)
    bad = [i for i in range(len(got)) if not gdi.group_ok(got[i], want_pts[i])]
    assert not bad, "%s: %d of %d leave the group, first at %d: %s" % (what, len(bad), len(got), bad[0], got[bad[0]])
    bad = [i for i in range(len(got)) if got[i] != model[i]]
    assert not bad, "%s: %d of %d differ from the formula, first at %d: got %s, expected %s" % (
        what, len(bad), len(got), bad[0], got[bad[0]], model[bad[0]])


# ---- XYZZ + XYZZ: add, add2 (dbl2), G1Quad::add (dbl) ------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    cases = gdi.pair_cases()
    got = gdi.kinds(cases, gdi.PAIR_KINDS)
    print("pair cases:", got)
    assert all(got[k] >= 8 for k in gdi.PAIR_KINDS), got
    ids = [c.p for c in cases if c.kind in ("p_id", "both_id")]
    assert IDENTITY in ids and any(p[2] == 0 and p[:2] != (1, 1) for p in ids)
    want = [gdi.log_sum([c.a, c.b]) for c in cases]
    model = [gdi.add(c.p, c.q) for c in cases]
    return cases, want, model


@pytest.mark.parametrize("op", [G_ADD, G_ADD2], ids=["add", "add2"])
def test_add(gdc, pairs, op):
    cases, want, model = pairs
    both_checks(gdc.points(op, [c.p for c in cases], [c.q for c in cases]), want, model, "add")


def _quad_copies(out, what):
    """(count, 64) words -> one XYZZ tuple per element, the four lanes' copies required equal."""
    lanes = gdi.unpack(out, 4)
    got = []
    for i in range(0, len(lanes), 4):
        assert lanes[i] == lanes[i + 1] == lanes[i + 2] == lanes[i + 3], "%s: lanes of quad %d differ" % (what, i // 4)
        got.append(lanes[i])
    return got


def test_quad_add(gdc, pairs):
    cases, want, model = pairs
    # 16 quads per wave: waves mix the exits, so a quad's exit cannot be its neighbours'
    exits = [gdi.exit_of(c) for c in cases]
    waves = [set(exits[i:i + 16]) for i in range(0, len(exits), 16)]
    assert sum(len(w) == 4 for w in waves) >= 3, waves
    assert sum(exits[i] != exits[i + 1] for i in range(len(exits) - 1)) >= len(exits) // 2
    out = gdc.run(Q_ADD, [c.p for c in cases], [c.q for c in cases])
    both_checks(_quad_copies(out, "G1Quad::add"), want, model, "G1Quad::add")


# ---- XYZZ + affine: madd, madd_tp --------------------------------------------------------------------
@pytest.mark.parametrize("op", [G_MADD, G_MADD_TP], ids=["madd", "madd_tp"])
def test_madd(gdc, op):
    cases = gdi.mixed_cases()
    got = gdi.kinds(cases, gdi.MIXED_KINDS)
    print("mixed cases:", got)
    assert all(got[k] >= 8 for k in gdi.MIXED_KINDS), got
    want = [gdi.log_sum([c.a, c.b]) for c in cases]
    model = [gdi.madd(c.p, c.q) for c in cases]
    both_checks(gdc.points(op, [c.p for c in cases], [c.q for c in cases]), want, model, "madd")


# ---- one operand: dbl, dbl2, G1Quad::dbl, mdbl, mul_small, to_affine_plain ----------------------
@pytest.fixture(scope="module")
def unary():
    cases = gdi.unary_cases()
    assert sum(a == 0 for _, a in cases) >= 6 and sum(p[2] == 1 for p, _ in cases) >= 8
    assert sum(p[2] > 1 for p, _ in cases) >= 16 and (IDENTITY, 0) in cases
    return cases


def test_dbl(gdc, unary):
    pts = [p for p, _ in unary]
    want = [gdi.log_sum([a, a]) for _, a in unary]
    model = [gdi.dbl(p) for p in pts]
    both_checks(gdc.points(G_DBL, pts), want, model, "dbl")
    both_checks(gdc.points(G_DBL2, pts), want, model, "dbl2")
    both_checks(_quad_copies(gdc.run(Q_DBL, pts), "G1Quad::dbl"), want, model, "G1Quad::dbl")
    aff = [(gdi.pt(a), a) for _, a in unary if a]
    both_checks(gdc.points(G_MDBL, [p for p, _ in aff]), [gdi.log_sum([a, a]) for _, a in aff],
                [gdi.mdbl(p) for p, _ in aff], "mdbl")


@pytest.mark.parametrize("k", gdi.MUL_SMALL_KS)
def test_mul_small(gdc, unary, k):
    import bn254

    pts = [p for p, _ in unary]
    model = [gdi.mul_small(p, k) for p in pts]
    # the formula restatement's own results are the group's (on the CPU, one oracle product each
    # for a few points; the rest follow coordinate for coordinate)
    want = [gdi.affine_of(m) for m in model]
    for (p, a), w in list(zip(unary, want))[:3]:
        assert w == (bn254.g1_mul(gdi.pt(a), k) if a and k else None)
    both_checks(gdc.points(G_MUL_SMALL, pts, p0=k), want, model, "mul_small(%d)" % k)


def test_to_affine_plain(gdc, unary):
    pts = [p for p, _ in unary]
    got = gdi.unpack(gdc.run(G_TO_AFFINE, pts), 2)
    assert got == [(0, 0) if a == 0 else gdi.pt(a) for _, a in unary]


# ---- the MSM's 29-bit-limb accumulator ----------------------------------------------------------------
@pytest.mark.parametrize("op", [ACC_XYZZ, ACC_RAW], ids=["to_xyzz", "raw"])
def test_accumulator_round_trip(gdc, unary, op):
    """to_xyzz(from_xyzz(p)) and raw_to_xyzz(store_raw(from_xyzz(p))) return p (canonical); with
    id = true both return G1::identity(), whatever the coordinates hold."""
    pts = [p for p, a in unary if a]
    assert len(pts) % 64 != 0
    out = gdi.unpack(gdc.run(op, pts), 4)
    assert out[0::2] == pts
    assert out[1::2] == [IDENTITY] * len(pts)


@pytest.mark.parametrize("k", [1, 2, 3, 5, gdi.MSM_CH])
def test_accumulation_chain(gdc, k):
    """The loop body of msm_chunk_acc_l29r (l29::madd; on true the point reloaded and
    acc = from_xyzz(G1::mdbl(q))) over K points from acc.id = true.

    The requirement is the group check: the sum of the discrete logs, through to_xyzz and through
    the raw round trip, and the two masks (which steps returned true, which left the identity)
    as predicted from the discrete logs. Coordinate equality with the same chain through
    G1::madd is asserted too: msm_l29.hpp keeps X, Y as x 2^261 and ZZ, ZZZ as x 2^266 of the
    very values madd-2008-s computes (the same formula, the same exits, the doubling by the same
    G1::mdbl), and to_xyzz multiplies the domain constants away and canonicalises, so the four
    coordinates are the same residues mod q."""
    items = gdi.chain_cases()[k]
    reps = 1
    while len(items) * reps % 64 == 0 or len(items) * reps < 3:
        reps += 1
    items = items * reps
    pts = [tuple(v for t in logs for v in gdi.pt(t)) for _, logs in items]
    want = [gdi.log_sum(logs) for _, logs in items]
    masks = [gdi.chain_masks_from_logs(logs) for _, logs in items]
    assert any(d for d, _ in masks) or k == 1
    assert any(i for _, i in masks) or k == 1
    models = [gdi.chain([gdi.pt(t) for t in logs])[0] for _, logs in items]
    out = gdc.run(ACC_CHAIN, pts, p0=k)
    via_to_xyzz = gdi.unpack(out[:, :16], 4)
    via_raw = gdi.unpack(out[:, 16:32], 4)
    for i, (name, _) in enumerate(items):
        assert (int(out[i, 32]), int(out[i, 33])) == masks[i], "%s: masks %#x %#x, predicted %#x %#x" % (
            (name, int(out[i, 32]), int(out[i, 33])) + masks[i])
    both_checks(via_to_xyzz, want, models, "l29 chain K=%d" % k)
    both_checks(via_raw, want, models, "l29 chain K=%d, raw round trip" % k)
    both_checks(gdc.points(G_CHAIN, pts, p0=k), want, models, "G1::madd chain K=%d" % k)
