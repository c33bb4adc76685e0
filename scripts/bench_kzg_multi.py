#!/usr/bin/env python3
"""Cost of the multi-point KZG opening (include/pbf.h "Multi-point KZG openings"), one process per
mode:

  open LOG_LEN     6 polynomials of 2^LOG_LEN coefficients, all opened at npts = 2, 4 and 8 points:
                   pbf_kzg_open_multi_bn254_dev + pbf_kzg_open_multi_finish_bn254_dev (two proof
                   points) against the yardstick, one pbf_kzg_open_bn254_dev per point (npts proof
                   points). The multi-opening is then verified once (it must be accepted).
  plonk LOG_LEN    the PLONK shape: 6 polynomials at z, one of them also at z omega; the yardstick
                   is the two plain openings (6 polynomials at z, 1 at z omega)
  verify           pbf_kzg_verify_multi_bn254 at count = 1, 256 and 4096 for 6 polynomials on 4
                   points (and the PLONK shape) against pbf_kzg_verify_bn254 with npts times as many
                   entries. The points are multiples of G and the evaluations random: both
                   verifiers run their whole path and answer 0.

--yardstick-lib PATH takes the yardstick from another build of libpbf.so (the parent commit's), in
its own context; without it the yardstick is this build's plain entry. Every path has a context
of its own, because the MSM's window table of the SRS is per context. Medians after a warm-up,
the paths alternating inside each repetition (the order rotates)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pbf  # noqa: E402
from bench_plonk_pi import Raw, alternate  # noqa: E402
from bench_prover import G2  # noqa: E402

S = 0x5EED0005C0FFEE
BATCH = 6
P = pbf._ptr


def rand_fr(count, seed):
    """count canonical values (below 2^252) as limbs."""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=4 * count, dtype=np.int64).astype(np.uint64)
    a[3::4] &= np.uint64((1 << 60) - 1)
    return a


def setup(length):
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    dsrs = torch.empty(length * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, length - 1, dsrs.data_ptr(), stream=sp)
    polys = torch.from_numpy(rand_fr(BATCH * length, 11).view(np.int64)).cuda()
    torch.cuda.synchronize()
    g2s = [G2, ctx.g2_bn254_mul([G2], [S])[0]]
    return ctx, sp, dsrs, polys, g2s


def multi_fn(c, dsrs, polys, length, batch, pts, sets, gamma, z, sp, out):
    npts = len(pts) // 4
    ys, w, w2 = np.zeros(4 * batch * npts, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    out.update(ys=ys, w=w, w2=w2)

    def fn():
        c.ok(c.lib.pbf_kzg_open_multi_bn254_dev(c.h, dsrs.data_ptr(), length, polys.data_ptr(), length, length, batch,
                                                P(pts), npts, P(sets), P(gamma), P(ys), P(w), sp))
        c.ok(c.lib.pbf_kzg_open_multi_finish_bn254_dev(c.h, dsrs.data_ptr(), length, polys.data_ptr(), length, length,
                                                       batch, P(pts), npts, P(sets), P(gamma), P(z), P(w2), sp))
    return fn


def plain_fn(c, dsrs, polys, length, calls, sp):
    """calls: (first polynomial, batch, point limbs, weight limbs) per plain opening"""
    outs = [(np.zeros(4 * b, np.uint64), np.zeros(8, np.uint64)) for _, b, _, _ in calls]

    def fn():
        for (b0, b, z, wts), (ys, w) in zip(calls, outs):
            c.ok(c.lib.pbf_kzg_open_bn254_dev(c.h, dsrs.data_ptr(), length, polys.data_ptr() + 32 * b0 * length, length,
                                              length, b, P(z), P(wts), P(ys), P(w), sp))
    return fn


def bench_open(log_len, ylib, shapes, reps=10):
    length = 1 << log_len
    ctx, sp, dsrs, polys, g2s = setup(length)
    print(f"# open: {BATCH} polynomials of 2^{log_len} coefficients, {reps} repetitions after a warm-up, yardstick = "
          f"plain openings of {os.path.basename(ylib) if ylib else 'this build'}, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the yardstick")
    gamma, z = rand_fr(1, 3), rand_fr(1, 4)
    for name, npts, sets in shapes:
        pts = rand_fr(npts, 20 + npts)
        sets_a = np.array(sets, dtype=np.uint64)
        cy, cm = Raw(ylib), Raw()
        calls = []
        for j in range(npts):  # one plain opening per point, over the polynomials that have it
            bs = [b for b in range(BATCH) if (sets[b] >> j) & 1]
            assert bs == list(range(bs[0], bs[-1] + 1))
            calls.append((bs[0], len(bs), pts[4 * j:4 * j + 4].copy(), rand_fr(len(bs), 30 + j)))
        out = {}
        alternate([(f"{name}: {npts} plain openings (yardstick)", plain_fn(cy, dsrs, polys, length, calls, sp)),
                   (f"{name}: multi open + finish", multi_fn(cm, dsrs, polys, length, BATCH, pts, sets_a, gamma, z, sp,
                                                             out))], reps)
        # the proof is accepted
        commits = ctx.kzg_commit_dev(dsrs.data_ptr(), length, polys.data_ptr(), length, length, BATCH)
        ok = ctypes.c_int(-1)
        cm.ok(cm.lib.pbf_kzg_verify_multi_bn254(cm.h, P(pbf._g2_limbs(g2s)), 1, BATCH, npts, P(sets_a),
                                                P(pbf._g1_limbs(commits)), P(pts), P(out["ys"]), P(gamma), P(z),
                                                P(out["w"]), P(out["w2"]), P(pbf.ints_to_limbs([1])), ctypes.byref(ok)))
        assert ok.value == 1, "the multi-opening was not accepted"
        cy.close()
        cm.close()
    ctx.close()


def bench_verify(ylib, reps=10):
    ctx = pbf.Context(0)
    g2l = pbf._g2_limbs([G2, ctx.g2_bn254_mul([G2], [S])[0]])
    srs1 = ctx.srs_create(S, 0)[:1]
    print(f"# verify: {reps} repetitions after a warm-up, yardstick = pbf_kzg_verify_bn254 of "
          f"{os.path.basename(ylib) if ylib else 'this build'}, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the yardstick")
    rng = np.random.default_rng(9)
    pool = []  # multiples of G
    for i in range(2):
        ks = [[int(x)] for x in rng.integers(1, 1 << 62, size=1 << 12)]
        pool += ctx.kzg_commit(srs1, ks)
    pool = pbf._g1_limbs(pool).reshape(-1, 8)
    take = lambda n, off: np.ascontiguousarray(pool[(np.arange(n) + off) % len(pool)]).reshape(-1)  # noqa: E731
    for name, npts, sets in (("6 polynomials on 4 points", 4, [15] * 6), ("PLONK shape", 2, [1, 1, 1, 1, 1, 3])):
        sets_a = np.array(sets, dtype=np.uint64)
        for count in (1, 256, 4096):
            cy, cm = Raw(ylib), Raw()
            ok = ctypes.c_int(-1)
            commits, w, w2 = take(count * BATCH, 0), take(count, 7), take(count, 99)
            pts = rand_fr(count * npts, 40)  # distinct with all but negligible probability
            y, gamma, z, rho = (rand_fr(n, 41 + i) for i, n in enumerate((count * BATCH * npts, count, count, count)))
            rho |= np.uint64(1)
            e = count * npts  # the plain entries: one per (opening, point)
            pc, pw, pz, py, prho = take(e, 3), take(e, 5), rand_fr(e, 50), rand_fr(e, 51), rand_fr(e, 52) | np.uint64(1)

            def yard():
                cy.ok(cy.lib.pbf_kzg_verify_bn254(cy.h, P(g2l), e, P(pc), P(pz), P(py), P(pw), P(prho), ctypes.byref(ok)))

            def multi():
                cm.ok(cm.lib.pbf_kzg_verify_multi_bn254(cm.h, P(g2l), count, BATCH, npts, P(sets_a), P(commits), P(pts),
                                                        P(y), P(gamma), P(z), P(w), P(w2), P(rho), ctypes.byref(ok)))

            alternate([(f"{name}, count {count}: {e} plain entries", yard),
                       (f"{name}, count {count}: multi verify", multi)], reps)
            cy.close()
            cm.close()
    ctx.close()


def main():
    args = sys.argv[1:]
    ylib = None
    if "--yardstick-lib" in args:
        i = args.index("--yardstick-lib")
        ylib = args[i + 1]
        del args[i:i + 2]
    mode = args[0] if args else "open"
    full = (1 << 8) - 1
    if mode == "open":
        bench_open(int(args[1]) if len(args) > 1 else 16, ylib,
                   [(f"npts = {k}", k, [full >> (8 - k)] * BATCH) for k in (2, 4, 8)])
    elif mode == "plonk":
        bench_open(int(args[1]) if len(args) > 1 else 16, ylib, [("PLONK shape", 2, [1, 1, 1, 1, 1, 3])])
    elif mode == "verify":
        bench_verify(ylib)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
