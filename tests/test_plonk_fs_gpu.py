"""Fiat-Shamir PLONK on the GPU (include/pbf.h "Fiat-Shamir": pbf_plonk_prove_bn254_fs*,
pbf_plonk_verify_bn254_fs*, pbf_plonk_verify_bn254_batch_fs*, pbf_plonk_circuit_digest_bn254*).

Expected values: the challenges come from the pure-Python model tests/transcript_expect.py applied to
the proof the library returned; the proof itself from the existing pbf_plonk_prove_bn254_pi fed those
challenges (code the transcript does not touch), whose own correctness tests/test_plonk_pi_gpu.py
holds against the oracle; the circuit digests of the golden circuits from
tests/golden/plonk_fs_bn254.json (the oracle's verification key), and at n = 1024 from kzg_commit
over the interpolated selector and sigma columns. Circuits, SRS and proofs are made once per module."""
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import plonk_pi_expect as E  # noqa: E402
import transcript_expect as T  # noqa: E402

pytestmark = pytest.mark.gpu
R = E.R
GOLD_FS = {(c["n"], c["npub"], c["mode"]): c
           for c in json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_fs_bn254.json")))["cases"]}
MODES = {"reference": 0, "paper": 1}
# (n, npub): the golden circuits, and scale_circuit at n = 1024 with a ragged three-level tree over pub
CASES = list(E.CASES) + [(1024, 257)]
IDS = [f"n{n}-npub{k}" for n, k in CASES]


def _pt(p):
    return None if p is None or tuple(p) == (0, 0) else tuple(p)


def _g2s(ctx, s):
    return [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [s])[0]]


def _g2s_coords(g2s):
    p = g2s[1]
    return [p[0][0], p[0][1], p[1][0], p[1][1]]


class World:
    """One circuit with its SRS, one statement and witness, the model's circuit digest."""

    def __init__(self, ctx, n, npub, mode, golden=None):
        self.ctx, self.n, self.npub, self.mode = ctx, n, npub, mode
        self.rng = random.Random(0xF5 + 64 * n + npub)
        if n <= 16 if golden is None else golden:
            c = E.case_inputs(n, npub, mode)
            self.q, self.cp, self.abc, self.pub, self.rnd = c["q"], c["copies"], c["abc"], c["pub"], c["rnd"]
            self.srs, self.g2s = ctx.srs_create(E.S_SECRET, 2 * n + 2), _g2s(ctx, E.S_SECRET)
            gold = GOLD_FS[(n, npub, mode)]
            self.vk = [_pt(p) for p in gold["vk"]]
            assert _g2s_coords(self.g2s) == gold["g2s"]
        else:
            s = self.rng.randrange(1, R)
            self.q, self.cp, self.a, self.b = E.scale_circuit(n, 0x5EED0500 + n)
            self.pub, self.abc = E.scale_statement(self.a, self.b, npub, 31)
            self.rnd = [self.rng.randrange(R) for _ in range(9)]
            self.srs, self.g2s = ctx.srs_create(s, 2 * n + 2 if mode == "reference" else n + 3), _g2s(ctx, s)
            self.vk = self._vk_by_commit()
        self.h0 = self.digest_model()

    def _vk_by_commit(self):
        """The 8 preprocessed commitments from kzg_commit over the interpolated columns: sigma label
        (kind, idx) is [1, k1, k2][kind] w^(idx - 1) (plonk.rs:181-189), k1 k2 = 2 3."""
        ctx, n, w = self.ctx, self.n, F.root_of_unity(self.n)
        pw = [1] * n
        for i in range(1, n):
            pw[i] = pw[i - 1] * w % R
        q_l, q_r, q_o, q_m, q_c = self.q
        sig = [[(1, 2, 3)[k] * pw[i - 1] % R for k, i in col] for col in self.cp]
        polys = [ctx.ntt_fr(w, list(col), inverse=True) for col in (q_m, q_l, q_r, q_o, q_c, *sig)]
        return [_pt(p) for p in ctx.kzg_commit(self.srs, polys)]

    def digest_model(self, k1=2, npub=None):
        return T.circuit_digest(MODES[self.mode], self.n, self.npub if npub is None else npub, k1, 3, self.vk,
                                _g2s_coords(self.g2s))

    def digest(self, k1k2=(2, 3), npub=None):
        return self.ctx.plonk_circuit_digest_bn254(self.q, self.cp, self.srs, self.g2s,
                                                   self.npub if npub is None else npub, k1k2, MODES[self.mode])

    def prove_fs(self, pub=None, abc=None, digest=None, ctx=None):
        pts, fs, ch = (ctx or self.ctx).plonk_prove_bn254_fs(self.q, self.cp, abc or self.abc,
                                                             self.pub if pub is None else pub, digest or self.h0,
                                                             self.rnd, self.srs, mode=MODES[self.mode])
        return [_pt(p) for p in pts], fs, ch

    def prove_pi(self, chal, pub=None, abc=None):
        pts, fs = self.ctx.plonk_prove_bn254_pi(self.q, self.cp, abc or self.abc, self.pub if pub is None else pub,
                                                chal, self.rnd, self.srs, mode=MODES[self.mode])
        return [_pt(p) for p in pts], fs

    def verify_fs(self, pts, fs, pub=None, k1k2=(2, 3)):
        return self.ctx.plonk_verify_bn254_fs(self.q, self.cp, self.srs, self.g2s, pts, fs,
                                              self.pub if pub is None else pub, k1k2, MODES[self.mode])


_WORLDS = {}


def world(ctx, n, npub, mode="paper"):
    key = (n, npub, mode)
    if key not in _WORLDS:
        w = World(ctx, n, npub, mode)
        w.proof = w.prove_fs()
        _WORLDS[key] = w
    return _WORLDS[key]


# ---------------------------------------------------------------- digest, challenges, the proof
@pytest.mark.parametrize("n,npub", CASES, ids=IDS)
def test_circuit_digest_is_the_models(ctx, n, npub):
    w = world(ctx, n, npub)
    if n <= 16:
        assert w.h0.hex() == GOLD_FS[(n, npub, "paper")]["digest"]
    try:
        for vk in (None, 0):
            ctx.set_option("verifier.vk", vk)
            assert w.digest() == w.h0
    finally:
        ctx.set_option("verifier.vk", None)
    assert w.digest(npub=npub - 1) == w.digest_model(npub=npub - 1) != w.h0
    assert w.digest(k1k2=(5, 3)) not in (w.h0, w.digest_model(k1=5))  # another k1 is other sigma commitments too


@pytest.mark.parametrize("mode", ["paper", "reference"])
@pytest.mark.parametrize("n,npub", CASES, ids=IDS)
def test_reported_challenges_are_the_models_and_prove_pi_returns_the_same_proof(ctx, n, npub, mode):
    w = world(ctx, n, npub, mode)
    pts, fs, ch = w.proof
    model, _ = T.proof_chain(w.h0, w.pub, pts, fs)
    assert ch == T.chal5(model) + [model["u"]]
    try:
        ctx.release_caches()
        assert w.prove_pi(ch[:5]) == (pts, fs), "key cold"
        assert w.prove_pi(ch[:5]) == (pts, fs), "key cached"
        assert w.prove_fs() == w.proof, "fs, key cached"
        ctx.set_option("prover.pk", 0)
        assert w.prove_pi(ch[:5]) == (pts, fs), "no key"
        assert w.prove_fs() == w.proof, "fs, no key"
    finally:
        ctx.set_option("prover.pk", None)


def test_prove_fs_without_public_inputs_and_device_form(ctx):
    import numpy as np
    import torch

    import pbf

    w = World(ctx, 1024, 0, "paper")
    pts, fs, ch = w.prove_fs()
    model, _ = T.proof_chain(w.h0, [], pts, fs)
    assert ch == T.chal5(model) + [model["u"]]
    assert ctx.plonk_prove_bn254(w.q, w.cp, w.abc, ch[:5], w.rnd, w.srs, mode=1) == (pts, fs)
    assert w.verify_fs(pts, fs) is True

    w = world(ctx, 1024, 257)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731
    d_q = dev(pbf.ints_to_limbs([x for col in w.q for x in col]))
    d_cp = dev(np.array([v for col in w.cp for (k, i) in col for v in (k, i)], dtype=np.uint64))
    d_abc = dev(pbf.ints_to_limbs([x for col in w.abc for x in col]))
    d_pub, d_srs = dev(pbf.ints_to_limbs(w.pub)), dev(pbf._g1_limbs(w.srs))
    args = (1024, d_q.data_ptr(), d_cp.data_ptr())
    vargs = args + (d_srs.data_ptr(), len(w.srs), w.g2s)
    assert ctx.plonk_circuit_digest_bn254_dev(*vargs, 257, mode=1) == w.h0
    p, f, c = ctx.plonk_prove_bn254_fs_dev(*args, d_abc.data_ptr(), d_pub.data_ptr(), 257, w.h0, w.rnd, d_srs.data_ptr(),
                                           len(w.srs), mode=1)
    ctx.sync()
    v = pbf.limbs_to_ints(p)
    assert ([_pt((v[2 * i], v[2 * i + 1])) for i in range(9)], pbf.limbs_to_ints(f), pbf.limbs_to_ints(c)) == w.proof
    wrong = [(w.pub[0] + 1) % R] + w.pub[1:]
    assert ctx.plonk_verify_bn254_fs_dev(*vargs, p, f, w.pub, mode=1) is True
    assert ctx.plonk_verify_bn254_fs_dev(*vargs, p, f, wrong, mode=1) is False
    assert ctx.plonk_verify_bn254_batch_fs_dev(*vargs, [(p, f)] * 2, [w.pub, wrong], mode=1, each=True) == \
        (False, [True, False])


# ---------------------------------------------------------------- the single verifier
@pytest.mark.parametrize("n,npub", CASES, ids=IDS)
def test_verify_fs_accepts_the_honest_proof_and_rejects_every_single_change(ctx, n, npub):
    w = world(ctx, n, npub)
    pts, fs, _ = w.proof
    assert w.verify_fs(pts, fs) is True
    other = _pt(w.srs[2])  # a curve point that is none of the proof's
    assert other not in pts
    for j in range(9):
        assert w.verify_fs(pts[:j] + [other] + pts[j + 1:], fs) is False, ("point", j)
    for j in range(7):
        assert w.verify_fs(pts, fs[:j] + [(fs[j] + 1) % R] + fs[j + 1:]) is False, ("field", j)
    bad = list(w.pub)
    bad[npub // 2] = (bad[npub // 2] + 1) % R
    assert w.verify_fs(pts, fs, pub=bad) is False
    assert w.verify_fs(pts, fs, pub=w.pub[:-1]) is False  # npub - 1: another digest, another P, another PI
    # a proof made under the digest of another k1: the verifier's digest comes from its own key
    p2, f2, _ = w.prove_fs(digest=w.digest(k1k2=(5, 3)))
    assert (p2, f2) != (pts, fs) and w.verify_fs(p2, f2) is False
    assert w.verify_fs(pts, fs) is True


# ---------------------------------------------------------------- batches
@pytest.fixture(scope="module")
def w16(ctx):
    """n = 16, npub = 5: eight statements of one circuit, each with its witness and its _fs proof."""
    w = World(ctx, 16, 5, "paper", golden=False)
    assert w.digest() == w.h0
    w.ents = []
    for k in range(8):
        pub, abc = E.scale_statement(w.a, w.b, 5, 500 + k)
        pts, fs, _ = w.prove_fs(pub=pub, abc=abc)
        w.ents.append({"pts": pts, "f": fs, "pub": pub, "abc": abc})
    return w


def _batch_fs(w, ents):
    return w.ctx.plonk_verify_bn254_batch_fs(w.q, w.cp, w.srs, w.g2s, [(e["pts"], e["f"]) for e in ents],
                                             [e["pub"] for e in ents], mode=1, each=True)


def _batch_plain(w, ents, chals, us, rhos):
    return w.ctx.plonk_verify_bn254_batch_pi(w.q, w.cp, w.srs, w.g2s, [(e["pts"], e["f"]) for e in ents],
                                             [e["pub"] for e in ents], chals, us, rhos, mode=1, each=True)


@pytest.mark.parametrize("count", [1, 5, 64])
def test_batch_fs_is_the_plain_batch_fed_the_models_challenges(w16, count):
    w = w16
    ents = [dict(w.ents[i % 8]) for i in range(count)]
    model = T.batch_challenges(w.h0, [e["pub"] for e in ents], [(e["pts"], e["f"]) for e in ents])
    assert _batch_fs(w, ents) == _batch_plain(w, ents, *model) == (True, [True] * count)
    assert w.ctx.plonk_verify_bn254_batch_fs(w.q, w.cp, w.srs, w.g2s, [(e["pts"], e["f"]) for e in ents],
                                             [e["pub"] for e in ents], mode=1) is True
    bad = count // 2
    ents[bad]["f"] = [(ents[bad]["f"][0] + 1) % R] + ents[bad]["f"][1:]
    model = T.batch_challenges(w.h0, [e["pub"] for e in ents], [(e["pts"], e["f"]) for e in ents])
    want = (False, [i != bad for i in range(count)])
    assert _batch_fs(w, ents) == _batch_plain(w, ents, *model) == want


def test_cancelling_errors_pass_the_plain_batch_with_equal_weights_and_fail_batch_fs(w16):
    """include/pbf.h, pbf_plonk_verify_bn254_batch: with predictable or equal weights the errors of two
    bad proofs can cancel. Two honest proofs under one set of caller-chosen challenges (one z), +D
    on the first W_z and -D on the second: E1 and E2 of the pair are unchanged."""
    w = w16
    chal, us = [w.rng.randrange(R) for _ in range(5)], [w.rng.randrange(R) for _ in range(2)]
    D = _pt(w.srs[3])
    ents = []
    for e in w.ents[:2]:
        pts, fs = w.prove_pi(chal, pub=e["pub"], abc=e["abc"])
        ents.append({"pts": pts, "f": fs, "pub": e["pub"]})
    assert _batch_plain(w, ents, [chal] * 2, us, [1, 1]) == (True, [True, True])
    ents[0]["pts"] = ents[0]["pts"][:7] + [B.g1_add(ents[0]["pts"][7], D)] + ents[0]["pts"][8:]
    ents[1]["pts"] = ents[1]["pts"][:7] + [B.g1_add(ents[1]["pts"][7], B.g1_neg(D))] + ents[1]["pts"][8:]
    # existing behaviour, asserted as such: the pair passes, each proof alone does not
    assert w.ctx.plonk_verify_bn254_batch_pi(w.q, w.cp, w.srs, w.g2s, [(e["pts"], e["f"]) for e in ents],
                                             [e["pub"] for e in ents], [chal] * 2, us, [1, 1], mode=1) is True
    assert _batch_plain(w, ents[:1], [chal], us[:1], [1]) == (False, [False])
    assert _batch_fs(w, ents) == (False, [False, False])
    # the same move on two honest _fs proofs: their weights come after the proofs
    ents = [dict(e) for e in w.ents[:2]]
    assert _batch_fs(w, ents) == (True, [True, True])
    ents[0]["pts"] = ents[0]["pts"][:7] + [B.g1_add(ents[0]["pts"][7], D)] + ents[0]["pts"][8:]
    ents[1]["pts"] = ents[1]["pts"][:7] + [B.g1_add(ents[1]["pts"][7], B.g1_neg(D))] + ents[1]["pts"][8:]
    assert _batch_fs(w, ents) == (False, [False, False])


# ---------------------------------------------------------------- errors and isolation
def test_argument_errors_and_a_following_plain_call(ctx):
    import ctypes

    import numpy as np

    import pbf

    w = world(ctx, 8, 2)
    pts, fs, ch = w.proof
    n, npub = 8, 2
    plain_before = w.prove_pi(ch[:5])
    assert plain_before == (pts, fs)

    def einval(call):
        with pytest.raises(pbf.PbfError) as ei:
            call()
        assert ei.value.code == pbf.PBF_EINVAL

    too_many = w.pub + [0] * (n + 1 - npub)
    not_canonical = [w.pub[0], R]
    both = [(pts, fs), (pts, fs)]
    for bad in (too_many, not_canonical):  # npub > n, a pub value >= r
        einval(lambda: w.prove_fs(pub=bad))
        einval(lambda: w.verify_fs(pts, fs, pub=bad))
    einval(lambda: ctx.plonk_verify_bn254_batch_fs(w.q, w.cp, w.srs, w.g2s, both, [too_many] * 2, mode=1))
    einval(lambda: ctx.plonk_verify_bn254_batch_fs(w.q, w.cp, w.srs, w.g2s, both, [w.pub, not_canonical], mode=1))
    einval(lambda: ctx.plonk_prove_bn254_fs(w.q, w.cp, w.abc, None, w.h0, w.rnd, w.srs, mode=1, npub=1))  # NULL pub
    einval(lambda: ctx.plonk_verify_bn254_fs(w.q, w.cp, w.srs, w.g2s, pts, fs, None, mode=1, npub=1))
    einval(lambda: ctx.plonk_verify_bn254_batch_fs(w.q, w.cp, w.srs, w.g2s, [], [], mode=1))  # count = 0
    einval(lambda: ctx.plonk_circuit_digest_bn254(w.q, w.cp, w.srs, w.g2s, n + 1, mode=1))
    # count > 2^20 and NULL pointers, straight at the C entry points (no array is read before the checks)
    qa, ca, sa = pbf._circuit_limbs(w.q, w.cp, w.srs)
    pa, fa = pbf._proof_limbs(pts, fs)
    g2, kk = pbf._g2_limbs(w.g2s), pbf.ints_to_limbs((2, 3))
    pb = pbf.ints_to_limbs(w.pub)
    ok = ctypes.c_int(-1)
    P = pbf._ptr
    head = (ctx.h, n, P(qa), P(ca), P(sa), len(w.srs), P(g2))
    assert ctx.lib.pbf_plonk_verify_bn254_batch_fs(*head, (1 << 20) + 1, P(pa), P(fa), P(pb), npub, P(kk), 1,
                                                   ctypes.byref(ok), None) == pbf.PBF_EINVAL
    assert ctx.lib.pbf_plonk_verify_bn254_batch_fs(*head, 1, None, P(fa), P(pb), npub, P(kk), 1, ctypes.byref(ok),
                                                   None) == pbf.PBF_EINVAL
    assert ctx.lib.pbf_plonk_verify_bn254_fs(*head, P(pa), None, P(pb), npub, P(kk), 1, ctypes.byref(ok)) == pbf.PBF_EINVAL
    assert ctx.lib.pbf_plonk_verify_bn254_fs(*head, P(pa), P(fa), P(pb), npub, P(kk), 1, None) == pbf.PBF_EINVAL
    aa = pbf.ints_to_limbs([x for col in w.abc for x in col])
    o1, o2 = np.zeros(72, dtype=np.uint64), np.zeros(28, dtype=np.uint64)
    assert ctx.lib.pbf_plonk_prove_bn254_fs(ctx.h, n, P(qa), P(ca), P(aa), P(pb), npub, None, P(pbf.ints_to_limbs(w.rnd)),
                                            P(kk), P(sa), len(w.srs), 1, P(o1), P(o2), None) == pbf.PBF_EINVAL
    assert ctx.lib.pbf_plonk_circuit_digest_bn254(*head, P(kk), 1, npub, None) == pbf.PBF_EINVAL
    # the context is as it was: the _fs calls and their errors changed no later plain call
    assert w.prove_fs() == w.proof and w.verify_fs(pts, fs) is True
    assert w.prove_pi(ch[:5]) == plain_before
    u = ch[5]
    assert ctx.plonk_verify_bn254_pi(w.q, w.cp, w.srs, w.g2s, pts, fs, w.pub, ch[:5], u, mode=1) is True
    assert ctx.plonk_verify_bn254_batch_pi(w.q, w.cp, w.srs, w.g2s, both, [w.pub] * 2, [ch[:5]] * 2, [u, u], [7, 8],
                                           mode=1, each=True) == (True, [True, True])


def test_an_fs_prove_does_not_disturb_the_plain_prover_on_a_fresh_context(ctx):
    import pbf

    w = world(ctx, 16, 5)
    chal = [w.rng.randrange(R) for _ in range(5)]
    first = w.prove_pi(chal)
    assert w.prove_fs() == w.proof
    assert w.prove_pi(chal) == first
    fresh = pbf.Context(0)
    try:
        assert w.prove_fs(ctx=fresh) == w.proof
    finally:
        fresh.close()
