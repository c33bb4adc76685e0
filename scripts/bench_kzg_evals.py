#!/usr/bin/env python3
"""KZG in evaluation form on one box: the G1 NTT (forward and inverse) and the opening from
evaluations, at n = 2^16 and 2^20; the median of REPS calls after a warm-up, with min - max.

  G1 NTT    pbf_ntt_g1_bn254_dev on [s^j]G. Group operations are counted as the code issues them:
            per twiddle product 1 doubling and 13 additions for the window table, 4 doublings per
            window below the scalar's top nonzero digit and one addition per further nonzero
            digit; 2 additions per butterfly; for the inverse one product by n^-1 per point.
            Printed beside it: the fixed-base MSM's accumulation rate from
            profiles/r06/msm_acc_clock.txt (2^20 points x 16 windows of mixed additions in
            1226.6 us), for the reader -- a different kernel doing a different operation.
  opening   pbf_kzg_open_evals_bn254_dev, batch 1 and 6, against what a caller of the parent
            commit does for the same (y, W): pbf_ntt_fr256_batch_dev(inverse) into a scratch
            copy, then pbf_kzg_open_bn254_dev. With --parent PATH that sequence runs on the parent
            commit's build of the library (a second copy loaded beside this one, with its own
            context), otherwise on this tree's. The two alternate inside every repetition; each
            side keeps its own context, so neither rebuilds the other's window table.

Without --step this is the driver: it never opens the GPU itself, runs each size as a child
process under its own time limit, stops at the first child that fails, and writes the children's
output to profiles/kzg_evals/bench.txt (--out).
Usage: bench_kzg_evals.py [--parent PATH] [--out FILE] [log2 n ...]   (default 16 20)"""
import argparse
import ctypes
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))

REPS, S = 7, 0x5EED0005C0FFEE
STEP_LIMIT_S = 420
MSM_ACC_RATE = (1 << 20) * 16 / 1226.6e-6  # mixed additions per second (profiles/r06/msm_acc_clock.txt)


def show(name, ts, extra=""):
    v = sorted(ts)
    print(f"{name:44s} | {v[len(v) // 2] * 1e3:10.3f} ms ({v[0] * 1e3:.3f} - {v[-1] * 1e3:.3f}){extra}")
    sys.stdout.flush()
    return v[len(v) // 2], v[-1] - v[0]


def count_group_ops(n, omega, inverse, R):
    """(doublings, additions) of one transform, from the digits of the twiddles it multiplies by."""
    import numpy as np

    h = n // 2
    w, pw = 1, []
    for _ in range(h):
        pw.append(w)
        w = w * omega % R
    import pbf

    limbs = pbf.ints_to_limbs(pw).reshape(h, 4)
    nz = np.zeros(h, dtype=np.int64)
    top = np.zeros(h, dtype=np.int64)
    for d in range(64):
        dig = (limbs[:, d // 16] >> np.uint64(4 * (d % 16))) & np.uint64(15)
        nz += dig != 0
        top = np.where(dig != 0, d, top)
    t = np.arange(h, dtype=np.int64)
    low = t & -t  # 2^v; twiddle index t is used by 2^(v+1) - 1 butterflies over the stages (t > 0)
    uses = np.where(t > 0, 2 * low - 1, 0)
    dbl = int((uses * (1 + 4 * top)).sum())
    add = int((uses * (13 + nz - 1)).sum()) + 2 * h * (n.bit_length() - 1)
    if inverse:
        ninv = pow(n, R - 2, R)
        digs = [(ninv >> (4 * d)) & 15 for d in range(64)]
        nzi, topi = sum(1 for x in digs if x), max(d for d, x in enumerate(digs) if x)
        dbl += n * (1 + 4 * topi)
        add += n * (13 + nzi - 1)
    return dbl, add


def step(lg, parent):
    import torch

    import pbf

    R = pbf.BN254_R
    n = 1 << lg
    omega = pow(5, (R - 1) // n, R)
    rng = random.Random(0xE7A15 + lg)
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# n = 2^{lg}, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max)")
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    dl = torch.empty_like(dsrs)
    fwd = torch.empty_like(dsrs)
    torch.cuda.synchronize()

    def timed(fn, reps=REPS):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    for inverse, out in ((False, fwd), (True, dl)):
        ts = timed(lambda: ctx.ntt_g1_dev(omega, dsrs.data_ptr(), out.data_ptr(), n, inverse=inverse, stream=sp))
        dbl, add = count_group_ops(n, omega, inverse, R)
        med = sorted(ts)[len(ts) // 2]
        show(f"G1 NTT 2^{lg} {'inverse' if inverse else 'forward'}", ts,
             f"  {dbl / 1e6:.1f} M dbl + {add / 1e6:.1f} M add = {(dbl + add) / med / 1e9:.2f} G group ops/s")
    print(f"#   for comparison: the fixed-base MSM accumulates {MSM_ACC_RATE / 1e9:.2f} G mixed additions/s "
          "(profiles/r06/msm_acc_clock.txt)")
    # dl is now the Lagrange SRS. The parent sequence on its own library and context.
    if parent:
        plib = ctypes.CDLL(parent)
        for name, res, args in pbf.SIGNATURES:
            if hasattr(plib, name):
                getattr(plib, name).restype, getattr(plib, name).argtypes = res, args
        ph = ctypes.c_void_p()
        assert plib.pbf_ctx_create(0, ctypes.byref(ph)) == 0
        pname = os.path.basename(parent)
    else:
        pctx = pbf.Context(0)
        plib, ph, pname = pctx.lib, pctx.h, "this tree's library"
    print(f"# opening: evaluation form on {os.path.basename(pbf.LIB_PATH)}, parent sequence on {pname}")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for batch in (1, 6):
        evals = torch.randint(-(1 << 63), (1 << 63) - 1, (batch * n, 4), dtype=torch.int64, device="cuda")
        evals[:, 3] &= (1 << 60) - 1  # canonical: below r's top limb
        coefs = torch.empty_like(evals)
        torch.cuda.synchronize()
        z = rng.randrange(R)
        weights = [rng.randrange(R) for _ in range(batch)]
        wl, zl, ol = pbf.ints_to_limbs(weights), pbf.ints_to_limbs([z]), pbf.ints_to_limbs([omega])
        got = {}

        def evals_open():
            got["e"] = ctx.kzg_open_evals_dev(dl.data_ptr(), n, omega, evals.data_ptr(), n, batch, z, weights, stream=sp)

        def parent_open():
            ys = pbf.ints_to_limbs([0] * batch)
            w = pbf.ints_to_limbs([0, 0])
            st = ctypes.c_void_p(sp) if sp else None
            rc = plib.pbf_ntt_fr256_batch_dev(ph, pbf._ptr(ol), vp(evals), vp(coefs), n, batch, 1, st)
            rc = rc or plib.pbf_kzg_open_bn254_dev(ph, vp(dsrs), n, vp(coefs), n, n, batch, pbf._ptr(zl), pbf._ptr(wl),
                                                   pbf._ptr(ys), pbf._ptr(w), st)
            assert rc == 0, plib.pbf_last_error()
            v = pbf.limbs_to_ints(w)
            got["p"] = (pbf.limbs_to_ints(ys), (v[0], v[1]))

        evals_open()
        parent_open()
        torch.cuda.synchronize()
        assert got["e"] == got["p"], "the two paths disagree"
        te, tp = [], []
        for _ in range(REPS):  # alternate inside every repetition
            for fn, ts in ((parent_open, tp), (evals_open, te)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
        pm, pspread = show(f"open 2^{lg} x {batch} parent: INTT + kzg_open", tp)
        em, _ = show(f"open 2^{lg} x {batch} from evaluations", te)
        verdict = "above" if em > pm + pspread else "within or below"
        print(f"#   evaluation form {em / pm:.2f} x the parent sequence: {verdict} its median + spread "
              f"({pspread * 1e3:.3f} ms); (y, W) identical")
        del evals, coefs
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_evals", "bench.txt"))
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("logs", nargs="*", type=int)
    a = ap.parse_args()
    if a.step is not None:
        step(a.step, a.parent)
        return 0
    lines = ["# scripts/bench_kzg_evals.py: KZG in evaluation form on one MI355X (DESIGN.md 3.10)"]
    rc = 0
    for lg in a.logs or [16, 20]:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", str(lg)]
        if a.parent:
            cmd += ["--parent", a.parent]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        lines += r.stdout.splitlines()
        if r.returncode:
            rc = r.returncode
            lines.append(f"# the 2^{lg} step ended with status {rc}: nothing further was run")
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
