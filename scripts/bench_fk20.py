#!/usr/bin/env python3
"""Every opening at once (FK20) on one box: the pointwise G1 product, the setup and
pbf_kzg_open_all_bn254_dev; the median of REPS calls after a warm-up, with min - max.

  product   pbf_g1_bn254_mul_dev at 2^14 and 2^17 random (point, scalar) pairs. Group operations
            are counted as the code issues them, from the scalars' digits, as
            scripts/bench_kzg_evals.py counts the butterflies': per product 1 doubling and 13
            additions for the window table, 4 doublings per window below the scalar's top nonzero
            digit and one addition per further nonzero digit.
  setup     pbf_kzg_fk20_setup_bn254_dev at n = 2^12 and 2^16.
  openings  pbf_kzg_open_all_bn254_dev at n = 2^12 and 2^16, batch 1 and 6, against single openings
            pbf_kzg_open_bn254_dev on the same polynomials at z = omega^i: all n of them at 2^12;
            at 2^16 the first 256, times 256 -- an extrapolation, labelled so. The two paths
            alternate inside every repetition, each on its own context, and their W are compared.
            The one condition (exit status 1 otherwise): at 2^12 the new call is faster than the n
            single openings by more than their min - max spread.
  split     at 2^16, the call's five steps timed between events on the public forms of the same
            steps (Fr NTT of size 2n, 2n products, inverse G1 NTT of size 2n, forward one of size
            n, Fr NTT of size n for y). The public forms end in affine conversions that the call
            itself skips, so the split is an upper bound of each share.

Without --step this is the driver: it never opens the GPU itself, runs each step as a child
process under its own time limit, stops at the first child that fails, and writes the children's
output to profiles/fk20/bench.txt (--out).
Usage: bench_fk20.py [--out FILE]"""
import argparse
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))

REPS, S = 7, 0x5EED0005C0FFEE
STEP_LIMIT_S = 420
STEPS = ["mul:14", "mul:17", "fk:12", "fk:16"]
SINGLES_AT_16 = 256


def show(name, ts, extra=""):
    v = sorted(ts)
    print(f"{name:46s} | {v[len(v) // 2] * 1e3:11.3f} ms ({v[0] * 1e3:.3f} - {v[-1] * 1e3:.3f}){extra}")
    sys.stdout.flush()
    return v[len(v) // 2], v[-1] - v[0]


def timed(torch, fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def random_fr(torch, count):
    """count canonical Fr values on the device (top limb below r's)."""
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda")
    t[:, 3] &= (1 << 60) - 1
    return t


def count_group_ops(scalars):
    """(doublings, additions) of the products by these scalars (a (count, 4) uint64 array)."""
    import numpy as np

    count = scalars.shape[0]
    nz = np.zeros(count, dtype=np.int64)
    top = np.zeros(count, dtype=np.int64)
    for d in range(64):
        dig = (scalars[:, d // 16] >> np.uint64(4 * (d % 16))) & np.uint64(15)
        nz += dig != 0
        top = np.where(dig != 0, d, top)
    some = nz > 0
    return int((some * (1 + 4 * top)).sum()), int((some * (13 + nz - 1)).sum())


def step_mul(lg):
    import numpy as np
    import torch

    import pbf

    n = 1 << lg
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# pointwise product, 2^{lg} pairs, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    pts = torch.empty(8 * n, dtype=torch.int64, device="cuda")
    es, ks = random_fr(torch, n), random_fr(torch, n)
    ctx.g1_mul_base_dev(es.data_ptr(), pts.data_ptr(), n, stream=sp)
    out = torch.empty_like(pts)
    torch.cuda.synchronize()
    ts = timed(torch, lambda: ctx.g1_mul_dev(pts.data_ptr(), ks.data_ptr(), out.data_ptr(), n, stream=sp))
    dbl, add = count_group_ops(ks.cpu().numpy().view(np.uint64))
    med = sorted(ts)[len(ts) // 2]
    show(f"g1_mul 2^{lg}", ts, f"  {dbl / 1e6:.1f} M dbl + {add / 1e6:.1f} M add = {(dbl + add) / med / 1e9:.2f} G group ops/s")
    print("#   for comparison: the butterfly stages of the G1 NTT issue 2.0 - 2.1 G group ops/s (DESIGN.md 3.10)")
    ctx.close()


def step_fk(lg):
    import torch

    import pbf

    R = pbf.BN254_R
    n = 1 << lg
    omega2 = pow(5, (R - 1) // (2 * n), R)
    omega = omega2 * omega2 % R
    rng = random.Random(0xF20 + lg)
    ctx, sctx = pbf.Context(0), pbf.Context(0)  # the new path and the single openings
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# n = 2^{lg}, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max)")
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    xext = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    show(f"fk20 setup 2^{lg}", timed(torch, lambda: ctx.kzg_fk20_setup_dev(dsrs.data_ptr(), n, omega2, n, xext.data_ptr(), stream=sp)))
    singles = n if lg <= 12 else SINGLES_AT_16
    scale = n // singles
    zs = [pow(omega, i, R) for i in range(singles)]
    ok = True
    for batch in (1, 6):
        polys = random_fr(torch, batch * n)
        d_y = torch.empty(4 * batch * n, dtype=torch.int64, device="cuda")
        d_w = torch.empty(8 * n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        weights = [rng.randrange(R) for _ in range(batch)]
        got = {}

        def open_all():
            ctx.kzg_open_all_dev(xext.data_ptr(), n, omega2, polys.data_ptr(), n, n, batch, weights, d_y.data_ptr(),
                                 d_w.data_ptr(), stream=sp)
            torch.cuda.synchronize()

        def open_singles():
            got["w"] = [sctx.kzg_open_dev(dsrs.data_ptr(), n, polys.data_ptr(), n, n, batch, z, weights, stream=sp)
                        for z in zs]

        open_all()
        open_singles()
        import numpy as np

        v = pbf.limbs_to_ints(d_w[:8 * singles].cpu().numpy().view(np.uint64))
        ys = pbf.limbs_to_ints(d_y.cpu().numpy().view(np.uint64))
        for i, (y1, w1) in enumerate(got["w"]):
            assert (v[2 * i], v[2 * i + 1]) == w1, f"W differs at i = {i}"
            assert [ys[b * n + i] for b in range(batch)] == y1, f"y differs at i = {i}"
        ta, ts = [], []
        for _ in range(REPS):  # alternate inside every repetition
            for fn, acc in ((open_singles, ts), (open_all, ta)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append(time.perf_counter() - t0)
        label = f"{singles} single openings" + (f" x {scale} (extrapolated)" if scale > 1 else "")
        sm, sspread = show(f"open 2^{lg} x {batch} {label}", [t * scale for t in ts])
        am, _ = show(f"open 2^{lg} x {batch} all at once", ta)
        faster = am < sm - sspread
        print(f"#   all at once {sm / am:.1f} x faster than the single openings; "
              f"{'beyond' if faster else 'NOT beyond'} their spread ({sspread * 1e3:.3f} ms); "
              f"y and W identical at the {singles} points compared")
        if lg <= 12 and not faster:
            ok = False
        del polys, d_y, d_w
    if lg >= 16:
        split(torch, pbf, ctx, n, omega2, omega, xext, sp)
    ctx.close()
    sctx.close()
    return 0 if ok else 1


def split(torch, pbf, ctx, n, omega2, omega, xext, sp):
    """The five steps on their public forms, between events on the stream."""
    c = random_fr(torch, n)
    bhat = torch.empty(2 * n * 4, dtype=torch.int64, device="cuda")
    y = torch.empty(n * 4, dtype=torch.int64, device="cuda")
    pts = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    out = torch.empty(8 * n, dtype=torch.int64, device="cuda")
    steps = [
        ("Fr NTT 2n (bhat)", lambda: ctx.ntt_fr_coset_batch_dev(omega2, 1, c.data_ptr(), n, bhat.data_ptr(), 2 * n, 1, stream=sp)),
        ("2n products", lambda: ctx.g1_mul_dev(xext.data_ptr(), bhat.data_ptr(), pts.data_ptr(), 2 * n, stream=sp)),
        ("inverse G1 NTT 2n", lambda: ctx.ntt_g1_dev(omega2, pts.data_ptr(), pts.data_ptr(), 2 * n, inverse=True, stream=sp)),
        ("forward G1 NTT n", lambda: ctx.ntt_g1_dev(omega, pts[8 * (n - 1):].data_ptr(), out.data_ptr(), n, stream=sp)),
        ("Fr NTT n (y)", lambda: ctx.ntt_fr_coset_batch_dev(omega, 1, c.data_ptr(), n, y.data_ptr(), n, 1, stream=sp)),
    ]
    for fn in (s[1] for s in steps):
        fn()
    torch.cuda.synchronize()
    acc = {name: [] for name, _ in steps}
    for _ in range(REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record()
        for k, (_, fn) in enumerate(steps):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        for k, (name, _) in enumerate(steps):
            acc[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e-3)
    total = sum(sorted(v)[len(v) // 2] for v in acc.values())
    print("# split of one call over its steps (public forms, between events; the inverse transform's public")
    print("# form also scales by (2n)^-1, 2n products the call does not make):")
    for name, v in acc.items():
        m, _ = show(f"  step: {name}", v)
        print(f"#     {100 * m / total:.1f} % of the five")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20", "bench.txt"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step is not None:
        kind, lg = a.step.split(":")
        return step_mul(int(lg)) if kind == "mul" else step_fk(int(lg))
    lines = ["# scripts/bench_fk20.py: every opening at once on one MI355X (DESIGN.md 3.11)"]
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
