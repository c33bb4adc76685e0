"""PLONK public inputs on the GPU (include/pbf.h "Public inputs": pbf_plonk_prove_bn254_pi*,
pbf_plonk_verify_bn254_pi*, pbf_plonk_verify_bn254_batch_pi*).

Expected values: the golden proofs of tests/golden/plonk_pi_bn254.json (from the unmodified oracle by
the derivation of tests/plonk_pi_expect.py), and at n = 1024 the existing plonk_prove_bn254 on q'
(q_c' = q_c - pub) transformed with kzg_open on PI's coefficients -- both from code the public
inputs do not touch. Circuits, SRS and proofs are made once per module."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import plonk_pi_expect as E  # noqa: E402

pytestmark = pytest.mark.gpu
R = E.R
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_pi_bn254.json")))["cases"]
IDS = [f"n{c['n']}-npub{c['npub']}-{c['mode']}" for c in GOLD]
MODES = {"reference": 0, "paper": 1}


def _g2s(ctx, s):
    return [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [s])[0]]


def _pt(p):
    return None if p is None or tuple(p) == (0, 0) else tuple(p)


@pytest.fixture(scope="module")
def gold_srs(ctx):
    """SRS and g2 of the golden cases, per n."""
    return {n: (ctx.srs_create(E.S_SECRET, 2 * n + 2), _g2s(ctx, E.S_SECRET)) for n in (8, 16)}


# ---------------------------------------------------------------- golden proofs
@pytest.mark.parametrize("case", GOLD, ids=IDS)
def test_golden_proofs_bit_for_bit_and_verified(ctx, gold_srs, case):
    n, npub, mode = case["n"], case["npub"], MODES[case["mode"]]
    c = E.case_inputs(n, npub, case["mode"])
    srs, g2s = gold_srs[n]
    want = ([_pt(p) for p in case["pts"]], case["fields"])

    def prove():
        pts, fs = ctx.plonk_prove_bn254_pi(c["q"], c["copies"], c["abc"], c["pub"], c["chal"], c["rnd"], srs, mode=mode)
        return [_pt(p) for p in pts], fs

    try:
        for l29 in (1, 0):
            ctx.set_option("ntt256.l29", l29)
            ctx.release_caches()
            assert prove() == want, ("key cold", l29)
            assert prove() == want, ("key cached", l29)
            ctx.set_option("prover.pk", 0)
            assert prove() == want, ("no key", l29)
            ctx.set_option("prover.pk", None)
    finally:
        ctx.set_option("prover.pk", None)
        ctx.set_option("ntt256.l29", None)
    if mode != 1:
        return

    def verify(pub):
        return ctx.plonk_verify_bn254_pi(c["q"], c["copies"], srs, g2s, want[0], want[1], pub, c["chal"], c["u"], mode=1)

    assert verify(c["pub"]) is True
    bad = list(c["pub"])
    bad[npub // 2] = (bad[npub // 2] + 1) % R
    assert verify(bad) is False
    other = E.case_inputs(n, npub, "reference")["pub"]  # the same circuit shape, another statement
    assert other != c["pub"] and verify(other) is False
    assert verify(c["pub"][:-1]) is False  # npub - 1 (npub = 1: none, the plain verifier)


# ---------------------------------------------------------------- one circuit, many statements
class World:
    """scale_circuit at n gates with its SRS; statements and their proofs on demand."""

    def __init__(self, ctx, n, seed):
        self.ctx, self.n, self.rng = ctx, n, random.Random(seed)
        self.s = self.rng.randrange(1, R)
        self.q, self.cp, self.a, self.b = E.scale_circuit(n, 0x5EED0500 + n)
        self.srs = ctx.srs_create(self.s, n + 3)
        self.g2s = _g2s(ctx, self.s)
        self.omega = F.root_of_unity(n)

    def statement(self, npub, seed, fixed=()):
        return E.scale_statement(self.a, self.b, npub, seed, fixed)

    def rand(self, k):
        return [self.rng.randrange(R) for _ in range(k)]

    def prove(self, pub, abc, chal, rnd, ctx=None):
        pts, fs = (ctx or self.ctx).plonk_prove_bn254_pi(self.q, self.cp, abc, pub, chal, rnd, self.srs, mode=1)
        return [_pt(p) for p in pts], fs

    def expected(self, pub, abc, chal, rnd):
        """The plain prover on q', then r_z and W_z moved by PI(z) and [v] commit of PI's opening
        quotient, which kzg_open returns for the weight v."""
        ctx = self.ctx
        pts, fs = ctx.plonk_prove_bn254(E.q_prime(self.q, pub), self.cp, abc, chal, rnd, self.srs, mode=1)
        pts = [_pt(p) for p in pts]
        if not pub:
            return pts, fs
        coeffs = ctx.ntt_fr(self.omega, [(-x) % R for x in pub] + [0] * (self.n - len(pub)), inverse=True)
        (y,), w = ctx.kzg_open(self.srs, [coeffs], chal[3], [chal[4]])
        fs[5] = (fs[5] - y) % R
        pts[7] = B.g1_add(pts[7], B.g1_neg(_pt(w)))
        return pts, fs

    def single(self, e, pub=None):
        return self.ctx.plonk_verify_bn254_pi(self.q, self.cp, self.srs, self.g2s, e["pts"], e["f"],
                                              e["pub"] if pub is None else pub, e["chal"], e["u"], mode=1)

    def batch(self, ents, each=True, pubs=None):
        return self.ctx.plonk_verify_bn254_batch_pi(
            self.q, self.cp, self.srs, self.g2s, [(e["pts"], e["f"]) for e in ents],
            [e["pub"] for e in ents] if pubs is None else pubs, [e["chal"] for e in ents], [e["u"] for e in ents],
            [e["rho"] for e in ents], mode=1, each=each)


@pytest.fixture(scope="module")
def w1024(ctx):
    return World(ctx, 1024, 10241)


@pytest.fixture(scope="module")
def w16(ctx):
    """n = 16, npub = 5: eight statements, each with its own witness, challenges and proof."""
    w = World(ctx, 16, 1605)
    w.proved = []
    for k in range(8):
        pub, abc = w.statement(5, 500 + k)
        chal, rnd = w.rand(5), w.rand(9)
        pts, fs = w.prove(pub, abc, chal, rnd)
        w.proved.append({"pts": pts, "f": fs, "pub": pub, "chal": chal})
    assert len({tuple(p["pub"]) for p in w.proved}) == 8

    def entries(count):
        return [dict(w.proved[i % 8], u=w.rng.randrange(R), rho=w.rng.randrange(1, R)) for i in range(count)]

    w.entries = entries
    return w


# ---------------------------------------------------------------- npub = 0 is the plain entry
@pytest.mark.parametrize("n", [8, 1024])
def test_npub_zero_is_the_plain_entry(ctx, n):
    w = World(ctx, n, 77 + n)
    _, abc = w.statement(0, 1)
    chal, rnd, u, rho = w.rand(5), w.rand(9), w.rng.randrange(R), w.rng.randrange(1, R)
    plain = ctx.plonk_prove_bn254(w.q, w.cp, abc, chal, rnd, w.srs, mode=1)
    assert ctx.plonk_prove_bn254_pi(w.q, w.cp, abc, [], chal, rnd, w.srs, mode=1) == plain
    assert ctx.plonk_prove_bn254_pi(w.q, w.cp, abc, None, chal, rnd, w.srs, mode=1) == plain
    pts, fs = plain
    tampered = [(fs[0] + 1) % R] + fs[1:]
    for f, want in ((fs, True), (tampered, False)):
        assert ctx.plonk_verify_bn254(w.q, w.cp, w.srs, w.g2s, pts, f, chal, u, mode=1) is want
        assert ctx.plonk_verify_bn254_pi(w.q, w.cp, w.srs, w.g2s, pts, f, None, chal, u, mode=1) is want
    proofs, chals = [(pts, fs), (pts, tampered), (pts, fs)], [chal] * 3
    us, rhos = [u, u + 1, u + 2], [rho, rho + 1, rho + 2]
    plain_b = ctx.plonk_verify_bn254_batch(w.q, w.cp, w.srs, w.g2s, proofs, chals, us, rhos, mode=1, each=True)
    assert plain_b == (False, [True, False, True])
    assert ctx.plonk_verify_bn254_batch_pi(w.q, w.cp, w.srs, w.g2s, proofs, [[]] * 3, chals, us, rhos, mode=1,
                                           each=True) == plain_b


# ---------------------------------------------------------------- lane and chunk edges
# the public-input kernels take 256 inputs per wave (4 per lane): 1 input, one short of a chunk, a
# full chunk, one input into the second chunk, four chunks (= n)
@pytest.mark.parametrize("npub", [1, 255, 256, 257, 1024])
def test_lane_and_chunk_edges_against_the_plain_prover_on_q_prime(ctx, w1024, npub):
    w = w1024
    pub, abc = w.statement(npub, 9000 + npub, fixed=((0, R - 1), (1, 0), (npub - 1, R - 1), (npub - 2, 0), (256, 0)))
    assert R - 1 in pub and (npub == 1 or 0 in pub)
    chal, rnd, u, rho = w.rand(5), w.rand(9), w.rng.randrange(R), w.rng.randrange(1, R)
    want = w.expected(pub, abc, chal, rnd)
    got = w.prove(pub, abc, chal, rnd)
    assert got[1] == want[1]
    assert got[0] == want[0]
    e = {"pts": got[0], "f": got[1], "pub": pub, "chal": chal, "u": u, "rho": rho}
    wrong = list(pub)
    wrong[npub - 1] = (wrong[npub - 1] + 1) % R
    try:
        for vk in (None, 0):
            ctx.set_option("verifier.vk", vk)
            assert w.single(e) is True
            assert w.single(e, wrong) is False
            assert w.batch([e]) == (True, [True])
            assert w.batch([e, e], pubs=[pub, wrong]) == (False, [True, False])
    finally:
        ctx.set_option("verifier.vk", None)


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).cuda()


def test_device_forms_agree_with_the_host_forms(ctx, w1024):
    import pbf

    w, n, npub = w1024, 1024, 257
    pub, abc = w.statement(npub, 4242)
    chal, rnd, u, rho = w.rand(5), w.rand(9), w.rng.randrange(R), w.rng.randrange(1, R)
    want = w.prove(pub, abc, chal, rnd)
    d_q = _dev(pbf.ints_to_limbs([x for col in w.q for x in col]))
    d_cp = _dev(np.array([v for col in w.cp for (k, i) in col for v in (k, i)], dtype=np.uint64))
    d_abc = _dev(pbf.ints_to_limbs([x for col in abc for x in col]))
    d_pub = _dev(pbf.ints_to_limbs(pub))
    d_srs = _dev(pbf._g1_limbs(w.srs))
    args = (n, d_q.data_ptr(), d_cp.data_ptr())
    pts, fs = ctx.plonk_prove_bn254_pi_dev(*args, d_abc.data_ptr(), d_pub.data_ptr(), npub, chal, rnd, d_srs.data_ptr(),
                                           len(w.srs), mode=1)
    ctx.sync()
    v = pbf.limbs_to_ints(pts)
    assert ([_pt((v[2 * i], v[2 * i + 1])) for i in range(9)], pbf.limbs_to_ints(fs)) == want
    wrong = [(pub[0] + 1) % R] + pub[1:]
    vargs = args + (d_srs.data_ptr(), len(w.srs), w.g2s)
    assert ctx.plonk_verify_bn254_pi_dev(*vargs, pts, fs, pub, chal, u, mode=1) is True
    assert ctx.plonk_verify_bn254_pi_dev(*vargs, pts, fs, wrong, chal, u, mode=1) is False
    assert ctx.plonk_verify_bn254_batch_pi_dev(*vargs, [(pts, fs)] * 2, [pub, wrong], [chal] * 2, [u, u + 1],
                                               [rho, rho + 1], mode=1, each=True) == (False, [True, False])
    # a device pub holding a value >= r: PBF_EINVAL from the constraint check's kernel
    d_bad = _dev(pbf.ints_to_limbs([R] + pub[1:]))
    with pytest.raises(pbf.PbfError) as ei:
        ctx.plonk_prove_bn254_pi_dev(*args, d_abc.data_ptr(), d_bad.data_ptr(), npub, chal, rnd, d_srs.data_ptr(),
                                     len(w.srs), mode=1)
    assert ei.value.code == pbf.PBF_EINVAL
    assert w.prove(pub, abc, chal, rnd) == want


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("count", [1, 3, 64, 65, 257])
def test_batches_of_distinct_statements(w16, count):
    ents = w16.entries(count)
    singles = [w16.single(e) for e in ents]
    assert singles == [True] * count
    assert w16.batch(ents) == (True, singles)
    assert w16.batch(ents, each=False) is True


def test_wrong_public_input_and_z_in_h_are_localised_among_65(w16):
    ents = w16.entries(65)
    bad = [dict(e) for e in ents]
    bad[17]["pub"] = list(bad[17]["pub"])
    bad[17]["pub"][4] = (bad[17]["pub"][4] + 1) % R
    bad[64]["chal"] = list(bad[64]["chal"])
    bad[64]["chal"][3] = w16.omega  # z = omega: a zero denominator in the public-input sum, Z_H(z) = 0
    want = [i not in (17, 64) for i in range(65)]
    assert [w16.single(bad[i]) for i in (16, 17, 63, 64)] == [True, False, True, False]
    assert w16.batch(bad) == (False, want)
    assert w16.batch(bad, each=False) is False


def test_valid_proof_under_another_entrys_statement_is_rejected(w16):
    ents = w16.entries(4)
    pubs = [e["pub"] for e in ents]
    pubs[1], pubs[2] = pubs[2], pubs[1]
    assert w16.batch(ents, pubs=pubs) == (False, [True, False, False, True])
    assert w16.single(ents[1], pubs[1]) is False


# ---------------------------------------------------------------- keys and isolation
def test_plain_and_pi_proves_do_not_disturb_each_other(ctx, w16):
    import pbf

    w = w16
    _, abc0 = w.statement(0, 1)
    chal, rnd = w.rand(5), w.rand(9)
    first = ctx.plonk_prove_bn254(w.q, w.cp, abc0, chal, rnd, w.srs, mode=1)
    stm = [w.statement(5, 70), w.statement(5, 71)]
    assert stm[0][0] != stm[1][0] and stm[0][1] != stm[1][1]
    here = [w.prove(pub, abc, chal, rnd) for pub, abc in stm]
    assert ctx.plonk_prove_bn254(w.q, w.cp, abc0, chal, rnd, w.srs, mode=1) == first
    assert here[0] != here[1]
    for (pub, abc), got in zip(stm, here):
        fresh = pbf.Context(0)
        try:
            assert w.prove(pub, abc, chal, rnd, ctx=fresh) == got
        finally:
            fresh.close()


# ---------------------------------------------------------------- errors
def test_argument_errors_leave_the_context_usable(ctx, gold_srs):
    import pbf

    n, npub = 8, 2
    case = next(c for c in GOLD if (c["n"], c["npub"], c["mode"]) == (n, npub, "paper"))
    c = E.case_inputs(n, npub, "paper")
    srs, g2s = gold_srs[n]
    want = ([_pt(p) for p in case["pts"]], case["fields"])

    def prove(pub, abc=c["abc"], npub=None):
        pts, fs = ctx.plonk_prove_bn254_pi(c["q"], c["copies"], abc, pub, c["chal"], c["rnd"], srs, mode=1, npub=npub)
        return [_pt(p) for p in pts], fs

    def verify(pub, npub=None):
        return ctx.plonk_verify_bn254_pi(c["q"], c["copies"], srs, g2s, want[0], want[1], pub, c["chal"], c["u"], mode=1,
                                         npub=npub)

    def batch(pub):
        return ctx.plonk_verify_bn254_batch_pi(c["q"], c["copies"], srs, g2s, [want, want], [c["pub"], pub],
                                               [c["chal"]] * 2, [5, 6], [7, 8], mode=1, each=True)

    def einval(call):
        with pytest.raises(pbf.PbfError) as ei:
            call()
        assert ei.value.code == pbf.PBF_EINVAL
        assert prove(c["pub"]) == want and verify(c["pub"]) is True
        assert batch(c["pub"]) == (True, [True, True])

    too_many = c["pub"] + [0] * (n + 1 - npub)
    not_canonical = [c["pub"][0], R]
    einval(lambda: prove(too_many))
    einval(lambda: prove(not_canonical))
    einval(lambda: prove(None, npub=1))
    a, b, w = c["abc"]
    assert c["q"][0][0] == 1 and a[0] == c["pub"][0]  # row 0 is a classic public row
    einval(lambda: prove(c["pub"], abc=([(a[0] + 1) % R] + a[1:], b, w)))
    einval(lambda: prove([(c["pub"][0] + 1) % R, c["pub"][1]]))  # the same row, seen from the statement
    einval(lambda: verify(too_many))
    einval(lambda: verify(not_canonical))
    einval(lambda: verify(None, npub=1))
    einval(lambda: batch(not_canonical))
    einval(lambda: ctx.plonk_verify_bn254_batch_pi(c["q"], c["copies"], srs, g2s, [want], [too_many], [c["chal"]], [5],
                                                   [7], mode=1))


# ---------------------------------------------------------------- the single verifier and a batch of one
# Both run plonk_verifier_scalars (csrc/plonk_terms.hpp), one on the host with rho = 1, one in
# k_vb_scalars: the same verdict, and the oracle's (tests/golden/plonk_verify_shapes.json, recorded
# from plonk_pi_expect.verify by tests/golden/gen_plonk_verify_shapes.py), at n = 8 and at n = 128,
# in both modes, without and with public inputs.
SHAPES = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_verify_shapes.json")))["cases"]


@pytest.fixture(scope="module")
def shape_srs(ctx):
    return {n: (ctx.srs_create(E.S_SECRET, n + 3), _g2s(ctx, E.S_SECRET)) for n in (8, 128)}


def test_shapes_cover_the_cases():
    assert [(c["n"], c["mode"], c["npub"]) for c in SHAPES] == \
        [(n, m, k) for n in (8, 128) for m in ("reference", "paper") for k in (0, 3)]
    assert all(c["s"] == E.S_SECRET and len(c["pub"]) == c["npub"] for c in SHAPES)


@pytest.mark.parametrize("case", SHAPES, ids=[f"n{c['n']}-npub{c['npub']}-{c['mode']}" for c in SHAPES])
def test_single_verifier_and_batch_of_one_give_the_oracles_verdict(ctx, shape_srs, case):
    n, mode, pub, chal, u = case["n"], MODES[case["mode"]], case["pub"], case["chal"], case["u"]
    q, cp, _a, _b = E.scale_circuit(n, case["seed"])
    srs, g2s = shape_srs[n]
    pts, fs = [_pt(p) for p in case["pts"]], case["fields"]
    rho = random.Random(case["seed"]).randrange(1, R)

    def verdict(pts=pts, fs=fs, chal=chal):
        """PBF_OK from both (an error would raise), and one verdict."""
        one = ctx.plonk_verify_bn254_pi(q, cp, srs, g2s, pts, fs, pub, chal, u, mode=mode)
        assert ctx.plonk_verify_bn254_batch_pi(q, cp, srs, g2s, [(pts, fs)], [pub], [chal], [u], [rho], mode=mode,
                                               each=True) == (one, [one])
        return one

    want = case["verdicts"]
    assert want["valid"] is (mode == 1)  # an honest reference-mode proof does not verify
    assert verdict() is want["valid"]
    assert verdict(fs=[(fs[0] + 1) % R] + fs[1:]) is want["a_z"] is False
    off = list(pts)
    off[7] = (off[7][0], (off[7][1] + 1) % B.Q)
    assert verdict(pts=off) is want["off_curve"] is False
    assert verdict(chal=chal[:3] + [F.root_of_unity(n)] + chal[4:]) is want["z_omega"] is False
