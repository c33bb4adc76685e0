#!/usr/bin/env python3
"""The batched G1 NTT and what runs on it, on one box: the median of REPS calls after a warm-up,
with min - max. In every comparison the two sides alternate inside every repetition, each on its
own context, and their results are compared for equality.

  ntt       pbf_ntt_g1_bn254_batch_dev against `batch` calls of pbf_ntt_g1_bn254_dev, forward, at
            n x batch = 2048 x 64, 128 x 64 and 2^16 x 4.
  setup     pbf_kzg_cells_setup_bn254_dev at (n, l) = (2^12, 64), (2^16, 64) and (2^16, 8) against the
            same call on the parent's library. Without --parent the parent's figures are quoted
            from profiles/fk20_cells/bench.txt and labelled as such.
  each      pbf_kzg_open_cells_each_bn254_dev against `batch` calls of pbf_kzg_open_cells_bn254_dev
            with weight 1, at (2^12, 64) and (2^16, 64), batch 1, 6 and 64. At (2^16, 64) x 64 also
            the one call under g1ntt.tile_log = 14, 16 and 18, and its split between events on the
            public forms of its steps: the batched Fr NTT of size 2k over batch x l rows and the two
            batched G1 transforms (these end in affine conversions, and the inverse in its scaling,
            which the call skips: upper bounds); the products and their sums are the call minus
            these, a lower bound.
  With --parent PATH the single calls and the parent's setup run on a libpbf.so built from the
  parent commit, as scripts/bench_kzg_evals.py does; else on a second context of this tree's.

Conditions (exit status 1 otherwise), the margins being the two min - max spreads together:
  (a) at (2^16, 64), batch 64, the one call is faster than the 64 calls;
  (b) the setup at (2^16, 64) is faster than the parent's;
  (c) at batch 1 the new call is not slower than the single call.

Without --step this is the driver: it never opens the GPU itself, runs each step as a child
process under its own time limit, stops at the first child that fails, and writes the children's
output to profiles/cells_each/bench.txt (--out).
Usage: bench_cells_each.py [--parent PATH] [--out FILE]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fk20 import REPS, S, random_fr, show  # noqa: E402

STEP_LIMIT_S = 420
STEPS = ["ntt", "setup", "each:12", "each:16", "tiles:16"]
QUOTED = os.path.join(ROOT, "profiles", "fk20_cells", "bench.txt")


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


def other_context(pbf, parent):
    """(context, name) of the side compared against: on the parent's library when one is given."""
    if not parent:
        return pbf.Context(0), "a second context of this tree's library"
    plib = ctypes.CDLL(parent)
    for name, res, args in pbf.SIGNATURES:
        if hasattr(plib, name):
            getattr(plib, name).restype, getattr(plib, name).argtypes = res, args
    c = pbf.Context.__new__(pbf.Context)
    c.lib, c.h, c.device = plib, ctypes.c_void_p(), 0
    assert plib.pbf_ctx_create(0, ctypes.byref(c.h)) == 0
    return c, "a libpbf.so built from the parent commit (--parent)"


def verdict(name, new, old, slower_ok=False):
    """new and old as (median, spread); the line of the report and whether the condition holds."""
    margin = new[1] + old[1]
    ok = new[0] <= old[0] + margin if slower_ok else new[0] < old[0] - margin
    print(f"#   {name}: {old[0] / new[0]:.2f} x; {'holds' if ok else 'DOES NOT HOLD'} beyond the two spreads together "
          f"({margin * 1e3:.3f} ms); results identical")
    return ok


def step_ntt(parent):
    import torch

    import pbf

    R = pbf.BN254_R
    ctx = pbf.Context(0)
    octx, oname = other_context(pbf, parent)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# batched G1 NTT, forward, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print(f"# the single calls run on {oname}")
    print("# path | median ms (min - max)")
    for n, batch in ((2048, 64), (128, 64), (1 << 16, 4)):
        omega = pow(5, (R - 1) // n, R)
        total = n * batch
        d_in = torch.empty(8 * total, dtype=torch.int64, device="cuda")
        ctx.srs_create_dev(S, total - 1, d_in.data_ptr(), stream=sp)  # any points will do
        one, many = (torch.empty(8 * total, dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()

        def batched():
            ctx.ntt_g1_batch_dev(omega, d_in.data_ptr(), one.data_ptr(), n, batch, stream=sp)

        def singles():
            for b in range(batch):
                octx.ntt_g1_dev(omega, d_in.data_ptr() + 64 * b * n, many.data_ptr() + 64 * b * n, n, stream=sp)

        batched()
        singles()
        torch.cuda.synchronize()
        assert torch.equal(one, many), "the transforms differ"
        ts, tb = alternate(torch, singles, batched)
        old = show(f"G1 NTT {n} x {batch}: {batch} single calls", ts)
        new = show(f"G1 NTT {n} x {batch}: one batched call", tb)
        verdict("batched against single", new, old)
    return 0


def quoted_setup(lg, l):
    """(median, spread) of the parent's setup from its committed report, or None."""
    try:
        text = open(QUOTED).read()
    except OSError:
        return None
    m = re.search(r"cells setup 2\^%d l=%d\s*\|\s*([\d.]+) ms \(([\d.]+) - ([\d.]+)\)" % (lg, l), text)
    return (float(m.group(1)) * 1e-3, (float(m.group(3)) - float(m.group(2))) * 1e-3) if m else None


def step_setup(parent):
    import torch

    import pbf

    R = pbf.BN254_R
    ctx = pbf.Context(0)
    octx, oname = other_context(pbf, parent) if parent else (None, None)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# cells setup, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print(f"# the parent's figures: {'measured on ' + oname if parent else 'QUOTED from profiles/fk20_cells/bench.txt, not measured in this run'}")
    ok = True
    for lg, l in ((12, 64), (16, 64), (16, 8)):
        n = 1 << lg
        omega2 = pow(5, (R - 1) // (2 * n), R)
        dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
        ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
        x_new, x_old = (torch.empty(16 * n, dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()

        def new_setup():
            ctx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, l, x_new.data_ptr(), stream=sp)

        def old_setup():
            octx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, l, x_old.data_ptr(), stream=sp)

        new_setup()
        if parent:
            old_setup()
            torch.cuda.synchronize()
            assert torch.equal(x_new, x_old), "xext differs"
            to, tn = alternate(torch, old_setup, new_setup)
            old = show(f"cells setup 2^{lg} l={l}: parent", to)
        else:
            _, tn = alternate(torch, lambda: None, new_setup)
            old = quoted_setup(lg, l)
            if old:
                print(f"{'cells setup 2^%d l=%d: parent (QUOTED)' % (lg, l):46s} | {old[0] * 1e3:11.3f} ms (spread {old[1] * 1e3:.3f})")
        new = show(f"cells setup 2^{lg} l={l}: batched", tn)
        if old:
            holds = verdict(f"setup 2^{lg} l={l}, batched against parent", new, old)
            if (lg, l) == (16, 64) and not holds:
                ok = False  # condition (b)
    return 0 if ok else 1


def each_inputs(torch, pbf, ctx, lg, l, sp):
    R = pbf.BN254_R
    n = 1 << lg
    omega2 = pow(5, (R - 1) // (2 * n), R)
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    xext = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, l, xext.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    return n, omega2, xext


def step_each(lg, parent):
    import torch

    import pbf

    l = 64
    ctx = pbf.Context(0)
    octx, oname = other_context(pbf, parent)
    sp = torch.cuda.current_stream().cuda_stream
    n, omega2, xext = each_inputs(torch, pbf, ctx, lg, l, sp)
    k = n // l
    print(f"# proofs of each polynomial, n = 2^{lg}, l = {l}, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}")
    print(f"# the single calls run on {oname}")
    ok = True
    for batch in (1, 6, 64):
        polys = random_fr(torch, batch * n)
        y1, y2 = (torch.empty(4 * batch * n, dtype=torch.int64, device="cuda") for _ in range(2))
        w1, w2 = (torch.empty(8 * batch * k, dtype=torch.int64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()

        def each():
            ctx.kzg_open_cells_each_dev(xext.data_ptr(), n, l, omega2, polys.data_ptr(), n, n, batch, y1.data_ptr(),
                                        w1.data_ptr(), stream=sp)

        def singles():
            for b in range(batch):
                octx.kzg_open_cells_dev(xext.data_ptr(), n, l, omega2, polys.data_ptr() + 32 * b * n, n, n, 1, [1],
                                        y2.data_ptr() + 32 * b * n, w2.data_ptr() + 64 * b * k, stream=sp)

        each()
        singles()
        torch.cuda.synchronize()
        assert torch.equal(w1, w2) and torch.equal(y1, y2) and bool(w1.any()), "the proofs differ"
        ts, te = alternate(torch, singles, each)
        old = show(f"cells 2^{lg} l={l} x {batch}: {batch} single calls", ts)
        new = show(f"cells 2^{lg} l={l} x {batch}: one call for each", te)
        holds = verdict(f"batch {batch}, one call against {batch}", new, old, slower_ok=batch == 1)
        if batch == 1 and not holds:
            ok = False  # condition (c)
        if batch == 64 and lg >= 16 and not holds:
            ok = False  # condition (a)
        del polys, y1, y2, w1, w2
    return 0 if ok else 1


def step_tiles(lg):
    """Batch 64 under three tiles, and the split of the call at the default one."""
    import torch

    import pbf

    R = pbf.BN254_R
    l, batch = 64, 64
    ctxs = {t: pbf.Context(0, options={"g1ntt.tile_log": str(t)}) for t in (14, 16, 18)}
    ctx = ctxs[14]
    sp = torch.cuda.current_stream().cuda_stream
    n, omega2, xext = each_inputs(torch, pbf, ctx, lg, l, sp)
    k = n // l
    print(f"# n = 2^{lg}, l = {l}, batch {batch} under g1ntt.tile_log = 14 (the default), 16 and 18, alternating; "
          f"{torch.cuda.get_device_name(0)}")
    polys = random_fr(torch, batch * n)
    ws = {t: torch.empty(8 * batch * k, dtype=torch.int64, device="cuda") for t in ctxs}
    torch.cuda.synchronize()
    call = {t: (lambda t=t: ctxs[t].kzg_open_cells_each_dev(xext.data_ptr(), n, l, omega2, polys.data_ptr(), n, n, batch, 0,
                                                            ws[t].data_ptr(), stream=sp)) for t in ctxs}
    for t in ctxs:
        call[t]()
    torch.cuda.synchronize()
    assert torch.equal(ws[14], ws[16]) and torch.equal(ws[14], ws[18]) and bool(ws[14].any()), "the proofs differ"
    acc = {t: [] for t in ctxs}
    for _ in range(REPS):
        for t in ctxs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call[t]()
            torch.cuda.synchronize()
            acc[t].append(time.perf_counter() - t0)
    res = {t: show(f"cells 2^{lg} l={l} x {batch}, tile_log {t}, no y", acc[t]) for t in ctxs}
    for t in (16, 18):
        verdict(f"tile_log {t} against 14", res[t], res[14])
    # the split at the default tile
    wl = pow(omega2, l, R)
    b_in = random_fr(torch, batch * n)
    bhat = torch.empty(4 * 2 * batch * n, dtype=torch.int64, device="cuda")
    pts = torch.empty(8 * batch * 2 * k, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, batch * 2 * k - 1, pts.data_ptr(), stream=sp)  # any points will do
    out = torch.empty(8 * batch * k, dtype=torch.int64, device="cuda")
    steps = [
        ("the whole call (no y)", call[14]),
        (f"Fr NTT 2k x {batch * l} rows (bhat)", lambda: ctx.ntt_fr_coset_batch_dev(wl, 1, b_in.data_ptr(), k, bhat.data_ptr(), 2 * k, batch * l, stream=sp)),
        (f"inverse G1 NTT 2k x {batch}", lambda: ctx.ntt_g1_batch_dev(wl, pts.data_ptr(), pts.data_ptr(), 2 * k, batch, inverse=True, stream=sp)),
        (f"forward G1 NTT k x {batch}", lambda: ctx.ntt_g1_batch_dev(wl * wl % R, pts.data_ptr(), out.data_ptr(), k, batch, stream=sp)),
    ]
    for _, fn in steps:
        fn()
    torch.cuda.synchronize()
    tm = {name: [] for name, _ in steps}
    for _ in range(REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record()
        for j, (_, fn) in enumerate(steps):
            fn()
            ev[j + 1].record()
        torch.cuda.synchronize()
        for j, (name, _) in enumerate(steps):
            tm[name].append(ev[j].elapsed_time(ev[j + 1]) * 1e-3)
    print("# split of one batch-64 call at the default tile (between events; the public forms are upper bounds of their steps):")
    med = {name: show(f"  step: {name}", v)[0] for name, v in tm.items()}
    total = med["the whole call (no y)"]
    rest = sum(m for name, m in med.items() if name != "the whole call (no y)")
    for name, m in med.items():
        if name != "the whole call (no y)":
            print(f"#     {name}: {100 * m / total:.1f} % of the call")
    print(f"#     products, gather and sums (the call minus the three steps): {(total - rest) * 1e3:.3f} ms, "
          f"{100 * (total - rest) / total:.1f} % of the call, {(total - rest) / batch * 1e3:.3f} ms per polynomial")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_each", "bench.txt"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step is not None:
        kind, _, lg = a.step.partition(":")
        if kind == "ntt":
            return step_ntt(a.parent)
        if kind == "setup":
            return step_setup(a.parent)
        return step_each(int(lg), a.parent) if kind == "each" else step_tiles(int(lg))
    lines = ["# scripts/bench_cells_each.py: the batched G1 NTT and the cell proofs of each polynomial on one MI355X "
             "(DESIGN.md 3.14)"]
    rc = 0
    for st in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", st]
        if a.parent:
            cmd += ["--parent", os.path.abspath(a.parent)]
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
