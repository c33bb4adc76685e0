#!/usr/bin/env python3
"""KZG cell proofs on one box: the setup, pbf_kzg_open_cells_bn254_dev against
pbf_kzg_open_all_bn254_dev, and the cell verifier against the point verifier; the median of REPS
calls after a warm-up, with min - max.

  setup     pbf_kzg_cells_setup_bn254_dev at n = 2^12 and 2^16, l = 64 and 8.
  cells     pbf_kzg_open_cells_bn254_dev at the same (n, l), batch 1 and 6, against
            pbf_kzg_open_all_bn254_dev at the same n on the same polynomials: the only way to prove
            the same data without cell proofs. The two paths alternate inside every repetition,
            each on its own context; the values y are compared (cell-major against natural order).
            The one condition (exit status 1 otherwise): at n = 2^16, l = 64 the new call is faster
            than open_all by more than the two min - max spreads together.
  split     at 2^16, the call between events, and its steps on their public forms: the batched Fr
            NTT of size 2k, the inverse G1 NTT of size 2k, the forward one of size k, the Fr NTT of
            size n for y. The public G1 forms end in affine conversions (and the inverse in 2k
            products by (2k)^-1) that the call skips, so each is an upper bound of its share. The
            products and their sum have no public form: they are the call minus the other steps, a
            lower bound, shown beside pbf_g1_bn254_mul_dev over the same 2n operands.
  verify    pbf_kzg_verify_cells_bn254 for 128 cells of 64 (n = 2^13) against pbf_kzg_verify_bn254
            over the same 8192 values as point openings whose proofs come from open_all; both on
            prebuilt arrays, alternating.

Without --step this is the driver: it never opens the GPU itself, runs each step as a child
process under its own time limit, stops at the first child that fails, and writes the children's
output to profiles/fk20_cells/bench.txt (--out).
Usage: bench_fk20_cells.py [--out FILE]"""
import argparse
import ctypes
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fk20 import REPS, S, random_fr, show, timed  # noqa: E402

STEP_LIMIT_S = 420
STEPS = ["cells:12", "cells:16", "verify:13"]
LS = (64, 8)


def alternate(torch, a, b):
    """REPS repetitions of a then b, each timed to its own synchronisation."""
    ta, tb = [], []
    for _ in range(REPS):
        for fn, acc in ((a, ta), (b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    return ta, tb


def step_cells(lg):
    import numpy as np
    import torch

    import pbf

    R = pbf.BN254_R
    n = 1 << lg
    omega2 = pow(5, (R - 1) // (2 * n), R)
    rng = random.Random(0xCE11 + lg)
    ctx, actx = pbf.Context(0), pbf.Context(0)  # the cell proofs and open_all
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# n = 2^{lg}, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max)")
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    x20 = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    actx.kzg_fk20_setup_dev(dsrs.data_ptr(), n, omega2, n, x20.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    ok = True
    for l in LS:
        k = n // l
        xext = torch.empty(16 * n, dtype=torch.int64, device="cuda")
        show(f"cells setup 2^{lg} l={l}",
             timed(torch, lambda: ctx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, l, xext.data_ptr(), stream=sp)))
        for batch in (1, 6):
            polys = random_fr(torch, batch * n)
            d_y = torch.empty(4 * batch * n, dtype=torch.int64, device="cuda")
            d_w = torch.empty(8 * k, dtype=torch.int64, device="cuda")
            a_y = torch.empty(4 * batch * n, dtype=torch.int64, device="cuda")
            a_w = torch.empty(8 * n, dtype=torch.int64, device="cuda")
            weights = [rng.randrange(R) for _ in range(batch)]

            def cells():
                ctx.kzg_open_cells_dev(xext.data_ptr(), n, l, omega2, polys.data_ptr(), n, n, batch, weights,
                                       d_y.data_ptr(), d_w.data_ptr(), stream=sp)

            def open_all():
                actx.kzg_open_all_dev(x20.data_ptr(), n, omega2, polys.data_ptr(), n, n, batch, weights, a_y.data_ptr(),
                                      a_w.data_ptr(), stream=sp)

            cells()
            open_all()
            torch.cuda.synchronize()
            # out_y[(b k + i) l + t] = y[b n + i + k t]
            assert torch.equal(d_y.view(batch, k, l, 4), a_y.view(batch, l, k, 4).transpose(1, 2)), "y differs"
            assert bool(d_w.any())
            ta, tc = alternate(torch, open_all, cells)
            am, aspread = show(f"open 2^{lg} x {batch} every point (open_all)", ta)
            cm, cspread = show(f"open 2^{lg} x {batch} cells of {l}", tc)
            faster = cm < am - (aspread + cspread)
            print(f"#   cells of {l}: {am / cm:.2f} x open_all; {'beyond' if faster else 'NOT beyond'} the two spreads "
                  f"together ({(aspread + cspread) * 1e3:.3f} ms); y identical")
            if lg >= 16 and l == 64 and not faster:
                ok = False
            del polys, d_y, d_w, a_y, a_w
        if lg >= 16:
            split(torch, pbf, ctx, n, l, omega2, xext, sp)
        del xext
    ctx.close()
    actx.close()
    return 0 if ok else 1


def split(torch, pbf, ctx, n, l, omega2, xext, sp):
    """The call between events, and its steps on their public forms."""
    R = pbf.BN254_R
    k = n // l
    wl, omega = pow(omega2, l, R), omega2 * omega2 % R
    c = random_fr(torch, n)
    bhat = torch.empty(2 * n * 4, dtype=torch.int64, device="cuda")
    y = torch.empty(n * 4, dtype=torch.int64, device="cuda")
    pts = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    out = torch.empty(8 * k, dtype=torch.int64, device="cuda")
    ctx.g1_mul_dev(xext.data_ptr(), c.repeat(2, 1).data_ptr(), pts.data_ptr(), 2 * n, stream=sp)  # points to transform
    torch.cuda.synchronize()
    steps = [
        ("the whole call", lambda: ctx.kzg_open_cells_dev(xext.data_ptr(), n, l, omega2, c.data_ptr(), n, n, 1, [1],
                                                           y.data_ptr(), out.data_ptr(), stream=sp)),
        (f"Fr NTT 2k x {l} (bhat)", lambda: ctx.ntt_fr_coset_batch_dev(wl, 1, c.data_ptr(), k, bhat.data_ptr(), 2 * k, l, stream=sp)),
        ("inverse G1 NTT 2k", lambda: ctx.ntt_g1_dev(wl, pts.data_ptr(), pts.data_ptr(), 2 * k, inverse=True, stream=sp)),
        ("forward G1 NTT k", lambda: ctx.ntt_g1_dev(wl * wl % R, pts[8 * (k - 1):].data_ptr(), out.data_ptr(), k, stream=sp)),
        ("Fr NTT n (y)", lambda: ctx.ntt_fr_coset_batch_dev(omega, 1, c.data_ptr(), n, y.data_ptr(), n, 1, stream=sp)),
        ("g1_mul over the 2n operands", lambda: ctx.g1_mul_dev(xext.data_ptr(), bhat.data_ptr(), pts.data_ptr(), 2 * n, stream=sp)),
    ]
    for fn in (s[1] for s in steps):
        fn()
    torch.cuda.synchronize()
    acc = {name: [] for name, _ in steps}
    for _ in range(REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record()
        for j, (_, fn) in enumerate(steps):
            fn()
            ev[j + 1].record()
        torch.cuda.synchronize()
        for j, (name, _) in enumerate(steps):
            acc[name].append(ev[j].elapsed_time(ev[j + 1]) * 1e-3)
    print(f"# split of one call, l = {l} (between events; public forms are upper bounds of their steps):")
    med = {}
    for name, v in acc.items():
        med[name], _ = show(f"  step: {name}", v)
    total = med["the whole call"]
    others = sum(m for name, m in med.items() if name not in ("the whole call", "g1_mul over the 2n operands"))
    for name, m in med.items():
        if name not in ("the whole call", "g1_mul over the 2n operands"):
            print(f"#     {name}: {100 * m / total:.1f} % of the call")
    print(f"#     products, gather and sum (the call minus the four steps): {(total - others) * 1e3:.3f} ms, "
          f"{100 * (total - others) / total:.1f} % of the call; g1_mul alone {med['g1_mul over the 2n operands'] * 1e3:.3f} ms")
    print(f"#     the two G1 transforms, of sizes {2 * k} and {k}, are launches of at most {k} lanes: "
          f"{100 * (med['inverse G1 NTT 2k'] + med['forward G1 NTT k']) / total:.1f} % of the call")


def step_verify(lg):
    import numpy as np
    import torch

    import pbf

    R = pbf.BN254_R
    n, l = 1 << lg, 64
    k = n // l
    omega2 = pow(5, (R - 1) // (2 * n), R)
    omega = omega2 * omega2 % R
    rng = random.Random(0x7E51F7)
    ctx, pctx = pbf.Context(0), pbf.Context(0)  # the cell verifier and the point verifier
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# verification, {k} cells of {l} (n = 2^{lg}), {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    poly = random_fr(torch, n)
    xc = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    x20 = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    y_c, y_p = (torch.empty(4 * n, dtype=torch.int64, device="cuda") for _ in range(2))
    w_c = torch.empty(8 * k, dtype=torch.int64, device="cuda")
    w_p = torch.empty(8 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, l, xc.data_ptr(), stream=sp)
    ctx.kzg_fk20_setup_dev(dsrs.data_ptr(), n, omega2, n, x20.data_ptr(), stream=sp)
    ctx.kzg_open_cells_dev(xc.data_ptr(), n, l, omega2, poly.data_ptr(), n, n, 1, [1], y_c.data_ptr(), w_c.data_ptr(), stream=sp)
    ctx.kzg_open_all_dev(x20.data_ptr(), n, omega2, poly.data_ptr(), n, n, 1, [1], y_p.data_ptr(), w_p.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    commit = ctx.kzg_commit_dev(dsrs.data_ptr(), n, poly.data_ptr(), n, n, 1)[0]
    u64 = lambda t: np.ascontiguousarray(t.cpu().numpy().view(np.uint64))  # noqa: E731
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from bn254_pairing import G2_GEN as g2

    g2l = ctx.g2_bn254_mul([g2, g2], [S % R, pow(S, l, R)])
    c_lim = pbf._g1_limbs([commit])
    ok = ctypes.c_int(-1)
    cell = dict(g2=pbf._g2_limbs([g2, g2l[1]]), srs=u64(dsrs[:8 * l]), om=pbf.ints_to_limbs([omega]),
                commits=np.tile(c_lim, k), idx=np.arange(k, dtype=np.uint64), ys=u64(y_c), w=u64(w_c),
                rho=pbf.ints_to_limbs([rng.randrange(1, R) for _ in range(k)]))
    point = dict(g2=pbf._g2_limbs([g2, g2l[0]]), commits=np.tile(c_lim, n), ys=u64(y_p), w=u64(w_p),
                 z=pbf.ints_to_limbs([pow(omega, i, R) for i in range(n)]),
                 rho=pbf.ints_to_limbs([rng.randrange(1, R) for _ in range(n)]))
    p = pbf._ptr

    def cells():
        rc = ctx.lib.pbf_kzg_verify_cells_bn254(ctx.h, p(cell["g2"]), p(cell["srs"]), l, p(cell["om"]), n, l, k,
                                                p(cell["commits"]), p(cell["idx"]), p(cell["ys"]), p(cell["w"]),
                                                p(cell["rho"]), ctypes.byref(ok))
        assert rc == 0 and ok.value == 1, (rc, ok.value)

    def points():
        rc = pctx.lib.pbf_kzg_verify_bn254(pctx.h, p(point["g2"]), n, p(point["commits"]), p(point["z"]), p(point["ys"]),
                                           p(point["w"]), p(point["rho"]), ctypes.byref(ok))
        assert rc == 0 and ok.value == 1, (rc, ok.value)

    cells()
    points()
    tp, tc = alternate(torch, points, cells)
    pm, _ = show(f"verify {n} point openings", tp)
    cm, _ = show(f"verify {k} cells of {l}", tc)
    print(f"#   the cell verifier takes {cm / pm:.2f} x the point verifier's time for the same {n} values, "
          f"with {k} proofs in place of {n}")
    ctx.close()
    pctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20_cells", "bench.txt"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step is not None:
        kind, lg = a.step.split(":")
        return step_cells(int(lg)) if kind == "cells" else step_verify(int(lg))
    lines = ["# scripts/bench_fk20_cells.py: KZG cell proofs on one MI355X (DESIGN.md 3.12)"]
    rc = 0
    for st in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", st]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        lines += r.stdout.splitlines()
        if r.returncode:
            rc = r.returncode
            lines.append(f"# the step {st} ended with status {rc}: nothing further was run")
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
