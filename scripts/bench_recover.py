#!/usr/bin/env python3
"""Recovery from cells on one box (pbf_kzg_recover_cells_bn254_dev); the median of
REPS calls after a warm-up, with min - max.

  rec       n = 2^13, 2^16 and 2^20 at l = 64, len = n/2, a random half of the cells known, batch
            1, 6 and 64, with and without out_y. Nothing in the library could do this before, so
            the yardstick is the three transforms the route cannot avoid, through their public
            entry points on a buffer of the same size: the batched inverse Fr NTT of size n, the
            forward coset transform and the inverse coset transform. The five paths alternate
            inside every repetition. The recovered coefficients, out_y and the flags are compared
            with the polynomials the cells were made from.
            The one condition (exit status 3 otherwise): at n = 2^16, l = 64, batch 64, without
            out_y, the call takes less than twice the sum of the three transforms.
            Stages: one call under context option recover.timing = 1, which synchronises at every
            stage mark: where the time goes, the Z values and their inversion first.
            (profiles/recover/bench_coset_route.txt is this script's log for the first version of
            the call, which went through the public coset transforms themselves.)
  zmax      k = 2^16, the supported maximum (n = 2^16, l = 1): the stages, for the product tree
            that would replace the direct products.
  open      n = 2^16, l = 64: recover, then pbf_kzg_open_cells_bn254_dev on the recovered
            coefficients, beside open_cells alone on the original ones.

Without --step this is the driver: it never opens the GPU itself, runs each step as a child
process under its own time limit, stops at the first child that fails (a missed condition is
reported and the remaining steps still run), and writes the children's
output to profiles/recover/bench.txt (--out).
Usage: bench_recover.py [--out FILE]"""
import argparse
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fk20 import REPS, S, random_fr, show  # noqa: E402

STEP_LIMIT_S = 300
STEPS = ["rec:13", "rec:16", "rec:20", "zmax:16", "open:16"]
L = 64
SHIFT = 5
MISSED = 3  # a step's exit status when it ran to its end and the condition was missed


def stages(torch, ctx, fn):
    """The stage times (ms) of one call under recover.timing = 1, from the library's stderr."""
    ctx.set_option("recover.timing", 1)
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tf:
        os.dup2(tf.fileno(), 2)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            ctx.set_option("recover.timing", None)
        tf.seek(0)
        text = tf.read().decode(errors="replace")
    out = []
    for line in text.splitlines():
        if line.startswith("[pbf recover]"):
            body = line[len("[pbf recover]"):].rsplit(None, 2)
            if len(body) == 3 and body[2] == "ms":
                out.append((body[0].strip(), float(body[1])))
    return out


def show_stages(st):
    total = sum(ms for _, ms in st)
    for name, ms in st:
        print(f"    stage: {name:38s} | {ms:11.3f} ms  {100 * ms / total:5.1f} %")
    print(f"    stage: {'sum (serialised by the marks)':38s} | {total:11.3f} ms")
    sys.stdout.flush()


class Case:
    """batch polynomials of n/2 coefficients, their cells, and the buffers of one call."""

    def __init__(self, torch, pbf, ctx, n, l, batch, seed):
        R = pbf.BN254_R
        self.torch, self.ctx, self.n, self.l, self.batch = torch, ctx, n, l, batch
        self.k, self.ln = n // l, n // 2
        self.omega = pow(5, (R - 1) // n, R)
        self.sp = torch.cuda.current_stream().cuda_stream
        rng = random.Random(seed)
        self.idx = rng.sample(range(self.k), self.k // 2)
        self.polys = random_fr(torch, batch * self.ln)
        self.work = torch.empty((batch * n, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.ntt_fr_coset_batch_dev(self.omega, 1, self.polys.data_ptr(), self.ln, self.work.data_ptr(), n, batch,
                                   stream=self.sp)
        torch.cuda.synchronize()
        # out_y[(b k + i) l + t] = y[b n + i + k t]
        self.want_y = self.work.view(batch, l, self.k, 4).transpose(1, 2).clone(memory_format=torch.contiguous_format)
        self.cells = self.want_y[:, torch.tensor(self.idx, device="cuda")].contiguous()
        self.d_p = torch.empty((batch * self.ln, 4), dtype=torch.int64, device="cuda")
        self.d_y = torch.empty((batch, self.k, l, 4), dtype=torch.int64, device="cuda")
        self.d_f = torch.empty(batch, dtype=torch.int32, device="cuda")

    def recover(self, with_y):
        self.ctx.kzg_recover_cells_dev(self.omega, self.n, self.l, self.ln, self.idx, self.cells.data_ptr(), self.batch,
                                       self.d_p.data_ptr(), self.ln, self.d_y.data_ptr() if with_y else 0,
                                       self.d_f.data_ptr(), stream=self.sp)

    def check(self):
        torch = self.torch
        self.d_p.fill_(-1)
        self.d_y.fill_(-1)
        self.d_f.fill_(-1)
        self.recover(True)
        torch.cuda.synchronize()
        assert torch.equal(self.d_p, self.polys), "the recovered coefficients differ"
        assert torch.equal(self.d_y, self.want_y), "out_y differs"
        assert bool((self.d_f == 1).all()), "a consistent input was flagged"


def step_rec(lg):
    import torch

    import pbf

    n = 1 << lg
    ctx = pbf.Context(0)
    print(f"# n = 2^{lg}, l = {L}, k = {n // L}, len = n/2, half the cells known; {REPS} repetitions after a warm-up, "
          f"{torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max)")
    ok = True
    for batch in (1, 6, 64):
        c = Case(torch, pbf, ctx, n, L, batch, 0x2EC0 + lg)
        c.check()
        w, om, sp = c.work.data_ptr(), c.omega, c.sp
        paths = [
            ("recover", lambda: c.recover(False)),
            ("recover with out_y", lambda: c.recover(True)),
            ("inverse Fr NTT", lambda: ctx.ntt_fr_batch_dev(om, w, w, n, batch, inverse=True, stream=sp)),
            ("forward coset Fr NTT", lambda: ctx.ntt_fr_coset_batch_dev(om, SHIFT, w, n, w, n, batch, stream=sp)),
            ("inverse coset Fr NTT", lambda: ctx.ntt_fr_coset_batch_dev(om, SHIFT, w, n, w, n, batch, inverse=True, stream=sp)),
        ]
        for _, fn in paths:
            fn()
        torch.cuda.synchronize()
        acc = {name: [] for name, _ in paths}
        for _ in range(REPS):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc[name].append(time.perf_counter() - t0)
        med = {name: show(f"2^{lg} x {batch}: {name}", v)[0] for name, v in acc.items()}
        three = med["inverse Fr NTT"] + med["forward coset Fr NTT"] + med["inverse coset Fr NTT"]
        print(f"#   2^{lg} x {batch}: the three transforms {three * 1e3:.3f} ms; recover = {med['recover'] / three:.2f} x, "
              f"with out_y {med['recover with out_y'] / three:.2f} x; results identical to the originals")
        if lg == 16 and batch == 64:
            met = med["recover"] < 2 * three
            print(f"#   the condition (recover < 2 x the three transforms): {'met' if met else 'MISSED'}")
            ok = ok and met
        st = stages(torch, ctx, lambda: c.recover(True))
        z = dict(st).get("Z values and inversion", float("nan"))
        print(f"#   2^{lg} x {batch}: Z values and their inversion {z:.3f} ms (between synchronisations)")
        show_stages(st)
        del c
    ctx.close()
    return 0 if ok else MISSED


def step_zmax(lg):
    import torch

    import pbf

    n = 1 << lg
    ctx = pbf.Context(0)
    print(f"# k = 2^{lg}, the supported maximum: n = 2^{lg}, l = 1, len = n/2, half the cells known, batch 1; "
          f"{torch.cuda.get_device_name(0)}")
    c = Case(torch, pbf, ctx, n, 1, 1, 0x2A11)
    c.check()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.recover(False)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    show(f"2^{lg} x 1, l = 1: recover", ts)
    show_stages(stages(torch, ctx, lambda: c.recover(False)))
    ctx.close()
    return 0


def step_open(lg):
    import torch

    import pbf

    R = pbf.BN254_R
    n = 1 << lg
    omega2 = pow(5, (R - 1) // (2 * n), R)
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# recover, then open_cells: n = 2^{lg}, l = {L}, len = n/2; {REPS} repetitions after a warm-up, "
          f"{torch.cuda.get_device_name(0)}")
    dsrs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    xext = torch.empty(16 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.srs_create_dev(S, n - 1, dsrs.data_ptr(), stream=sp)
    ctx.kzg_cells_setup_dev(dsrs.data_ptr(), n, omega2, n, L, xext.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    for batch in (1, 6):
        c = Case(torch, pbf, ctx, n, L, batch, 0x0BE2 + batch)
        assert c.omega == omega2 * omega2 % R
        c.check()
        rng = random.Random(batch)
        weights = [rng.randrange(R) for _ in range(batch)]
        w_a, w_b = (torch.empty(8 * c.k, dtype=torch.int64, device="cuda") for _ in range(2))

        def open_cells(d_polys, d_w):
            ctx.kzg_open_cells_dev(xext.data_ptr(), n, L, omega2, d_polys.data_ptr(), c.ln, c.ln, batch, weights, 0,
                                   d_w.data_ptr(), stream=sp)

        def alone():
            open_cells(c.polys, w_a)

        def both():
            c.recover(True)
            open_cells(c.d_p, w_b)

        alone()
        both()
        torch.cuda.synchronize()
        assert torch.equal(w_a, w_b) and bool(w_a.any()), "the proofs differ"
        ta, tb = [], []
        for _ in range(REPS):
            for fn, acc in ((alone, ta), (both, tb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        am, _ = show(f"2^{lg} x {batch}: open_cells alone", ta)
        bm, _ = show(f"2^{lg} x {batch}: recover with out_y, then open_cells", tb)
        print(f"#   2^{lg} x {batch}: recovery adds {(bm - am) * 1e3:.3f} ms, {100 * (bm - am) / am:.1f} % of the proofs; "
              f"proofs identical")
        del c
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover", "bench.txt"))
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step is not None:
        kind, lg = a.step.split(":")
        return {"rec": step_rec, "zmax": step_zmax, "open": step_open}[kind](int(lg))
    lines = ["# scripts/bench_recover.py: recovery from cells on one MI355X (DESIGN.md 3.13)"]
    rc = 0
    for st in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", st]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stderr.write(r.stderr)
        lines += r.stdout.splitlines()
        if r.returncode == MISSED:
            rc = MISSED
            lines.append(f"# the step {st} missed its condition")
        elif r.returncode:
            rc = r.returncode
            lines.append(f"# the step {st} ended with status {rc}: nothing further was run")
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
