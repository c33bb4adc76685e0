"""Batched Plonk::verify (csrc/verify_batch.hip, pbf_plonk_verify_bn254_batch) against the single
verifier: one random linear combination of the KZG checks per batch, structural rejection, and
localisation by halving. Proofs are made once per module at n = 8 and 16 (paper mode); larger
batches repeat them with distinct u_i and rho_i."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import plonk_bn254 as P  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_bn254.json")))["cases"]
MODES = {"reference": 0, "paper": 1}


class World:
    """One circuit and SRS at n gates, `k` distinct valid paper-mode proofs."""

    def __init__(self, ctx, n, k, seed):
        rng = random.Random(seed)
        self.n, self.ctx, self.rng = n, ctx, rng
        s = rng.randrange(1, P.R)
        self.q, self.cp, abc = P.mul_gates_circuit(n, 0xBA7C0000 + n)
        self.srs = ctx.srs_create(s, n + 3)
        self.g2s = [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [s])[0]]
        self.chals, self.proofs = [], []
        for _ in range(k):
            chal = [rng.randrange(P.R) for _ in range(5)]
            rnd = [rng.randrange(P.R) for _ in range(9)]
            self.chals.append(chal)
            self.proofs.append(ctx.plonk_prove_bn254(self.q, self.cp, abc, chal, rnd, self.srs, mode=1))

    def entries(self, count):
        """count entries cycling through the proofs, each with its own u and rho."""
        k = len(self.proofs)
        return [{"pts": list(self.proofs[i % k][0]), "f": list(self.proofs[i % k][1]), "chal": list(self.chals[i % k]),
                 "u": self.rng.randrange(P.R), "rho": self.rng.randrange(1, P.R)} for i in range(count)]

    def batch(self, ents, each=True, srs=None, rhos=None):
        return self.ctx.plonk_verify_bn254_batch(
            self.q, self.cp, self.srs if srs is None else srs, self.g2s, [(e["pts"], e["f"]) for e in ents],
            [e["chal"] for e in ents], [e["u"] for e in ents], [e["rho"] for e in ents] if rhos is None else rhos,
            mode=1, each=each)

    def single(self, e):
        return self.ctx.plonk_verify_bn254(self.q, self.cp, self.srs, self.g2s, e["pts"], e["f"], e["chal"], e["u"],
                                           mode=1)


@pytest.fixture(scope="module")
def w16(ctx):
    return World(ctx, 16, 3, 1601)


@pytest.fixture(scope="module")
def w8(ctx):
    return World(ctx, 8, 2, 801)


@pytest.fixture(scope="module")
def base65(w16):
    """65 valid entries and the single verifier's answer for each (all True)."""
    ents = w16.entries(65)
    singles = [w16.single(e) for e in ents]
    assert all(singles)
    return ents, singles


@pytest.mark.parametrize("case", GOLD, ids=[f"n{c['n']}-{c['mode']}" for c in GOLD])
def test_golden_single_proof_batches(ctx, case):
    q, cp, _ = P.mul_gates_circuit(case["n"], case["circuit_seed"])
    srs = ctx.srs_create(case["s"], case["srs_n"])
    g2s = [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [case["s"]])[0]]
    pts = [tuple(p) if p else None for p in case["pts"]]
    mode = MODES[case["mode"]]
    rho = random.Random(case["n"] + mode).randrange(1, P.R)
    single = ctx.plonk_verify_bn254(q, cp, srs, g2s, pts, case["fields"], case["chal"], case["u"], mode=mode)
    ok, each = ctx.plonk_verify_bn254_batch(q, cp, srs, g2s, [(pts, case["fields"])], [case["chal"]], [case["u"]],
                                            [rho], mode=mode, each=True)
    assert ok == case["verify"] == single
    assert each == [single]
    assert ctx.plonk_verify_bn254_batch(q, cp, srs, g2s, [(pts, case["fields"])], [case["chal"]], [case["u"]], [rho],
                                        mode=mode) == single


@pytest.mark.parametrize("count", [2, 3, 63, 64, 65, 257])
def test_valid_batches_across_wave_and_block_sizes(ctx, w8, w16, count):
    w = w8 if count < 4 else w16
    ents = w.entries(count)
    assert w.batch(ents) == (True, [True] * count)
    assert w.batch(ents, each=False) is True
    ctx.set_option("verifier.vk", 0)
    try:
        assert w.batch(ents) == (True, [True] * count)
    finally:
        ctx.set_option("verifier.vk", None)


def _tamper(w, e, kind):
    e = {k: (list(v) if isinstance(v, list) else v) for k, v in e.items()}
    if kind == "a_z+1":
        e["f"][0] = (e["f"][0] + 1) % P.R
    elif kind == "w_z=2G":
        e["pts"][7] = F.g1_mul(F.G1_GEN, 2)
    elif kind == "off-curve":
        x, y = e["pts"][0]
        e["pts"][0] = (x, (y + 1) % F.Q)
        assert not F.g1_on_curve(e["pts"][0])
    elif kind == "field=r":
        e["f"][2] = P.R
    elif kind == "z=omega":
        e["chal"][3] = F.root_of_unity(w.n)
    return e


@pytest.mark.parametrize("kind", ["a_z+1", "w_z=2G", "off-curve", "field=r", "z=omega"])
def test_one_bad_proof_among_65_is_localised(w16, base65, kind):
    ents, singles = base65
    for pos in (0, 63, 64):
        bad = list(ents)
        bad[pos] = _tamper(w16, ents[pos], kind)
        want = list(singles)  # the other 64 entries are untouched: their answers cannot differ
        want[pos] = w16.single(bad[pos])
        assert want[pos] is False
        ok, each = w16.batch(bad)
        assert ok is False
        assert each == want, (kind, pos)
        assert w16.batch(bad, each=False) is False


def test_weights_are_applied_and_the_check_is_combined(w16):
    e = w16.entries(1)[0]
    g = F.G1_GEN
    plus, minus = dict(e), dict(e)
    plus["pts"] = list(e["pts"])
    minus["pts"] = list(e["pts"])
    plus["pts"][7] = F.g1_add(e["pts"][7], g)
    minus["pts"][7] = F.g1_add(e["pts"][7], F.g1_mul(g, P.R - 1))
    assert F.g1_on_curve(plus["pts"][7]) and F.g1_on_curve(minus["pts"][7])
    pair = [plus, minus]
    assert [w16.single(x) for x in pair] == [False, False]
    rho = w16.rng.randrange(1, P.R)
    # equal weights: the +G and -G terms cancel in sum rho E1 and in sum rho z W_z
    assert w16.batch(pair, rhos=[rho, rho]) == (True, [True, True])
    # distinct weights: the defect e(G, G2)^((rho_0 - rho_1)(s - z)) != 1 shows
    assert w16.batch(pair, rhos=[1, 2]) == (False, [False, False])


def test_argument_errors_leave_the_context_usable(w8):
    import pbf

    ents = w8.entries(3)

    def einval(call):
        with pytest.raises(pbf.PbfError) as ei:
            call()
        assert ei.value.code == pbf.PBF_EINVAL
        assert w8.batch(ents) == (True, [True] * 3)

    einval(lambda: w8.batch([]))
    einval(lambda: w8.batch(ents, rhos=[5, 0, 7]))
    einval(lambda: w8.batch(ents, rhos=[5, 6, P.R]))
    einval(lambda: w8.batch(ents, srs=w8.srs[:w8.n - 1]))


def test_verification_key_is_shared_with_the_single_verifier(w16):
    ents = w16.entries(5)
    bad = _tamper(w16, ents[1], "a_z+1")
    assert w16.single(ents[0]) and not w16.single(bad)
    assert w16.batch(ents) == (True, [True] * 5)
    assert w16.batch([ents[0], bad, ents[2]]) == (False, [True, False, True])
    assert w16.single(ents[0]) and not w16.single(bad)
