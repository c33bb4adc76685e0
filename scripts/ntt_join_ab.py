#!/usr/bin/env python3
"""Alternation of library builds on the headline workload (32 x 2^20 forward Goldilocks NTT), every
run a fresh process of bench.py, in two windows:
  plain  = bench.py --steps 20 --warmup 5 (the driver's window);
  steady = bench.py --steps 100 --warmup 200 (steady clocks).

  python scripts/ntt_join_ab.py [--rounds 7] [--log-n 20] [--batch 32] label=lib.so[,ENV=VALUE...] ...

The first build is the parent. Every round runs each build once per window, in the order given.
Prints the raw ms per step of every run, per build the median / min / max, and for every other
build against the parent: the ratio of medians, whether every run is faster than every parent
run, and the keep rule (every run faster than every parent run in at least one window, the
median not above the parent's in the other). Stops at the first run that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (("plain", 20, 5), ("steady", 100, 200))


def one_run(lib, env_extra, steps, warmup, log_n, batch):
    env = dict(os.environ, PBF_LIB=os.path.join(ROOT, lib), **env_extra)
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
           str(steps), "--warmup", str(warmup), "--log-n", str(log_n), "--batch", str(batch)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"bench.py failed with {p.returncode} on {lib} {env_extra}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("builds", nargs="+")
    args = ap.parse_args()
    builds = []
    for spec in args.builds:
        label, rest = spec.split("=", 1)
        parts = rest.split(",")
        builds.append((label, parts[0], dict(kv.split("=", 1) for kv in parts[1:])))
    runs = {(w[0], b[0]): [] for w in WINDOWS for b in builds}
    for r in range(args.rounds):
        for wname, steps, warmup in WINDOWS:
            for label, lib, env in builds:
                ms = one_run(lib, env, steps, warmup, args.log_n, args.batch)
                runs[(wname, label)].append(ms)
                print(f"round {r} {wname:6s} {label:12s} {ms:.4f}", flush=True)
    print(f"# {args.batch} x 2^{args.log_n}, {args.rounds} rounds, ms per step; builds: "
          + "; ".join(f"{lb} = {lib} {env or ''}".strip() for lb, lib, env in builds))
    med = {}
    for wname, _, _ in WINDOWS:
        for label, _, _ in builds:
            v = runs[(wname, label)]
            med[(wname, label)] = statistics.median(v)
            print(f"{wname:6s} {label:12s} runs {[round(x, 4) for x in v]}  median {statistics.median(v):.4f} "
                  f"min {min(v):.4f} max {max(v):.4f}")
    parent = builds[0][0]
    for label, _, _ in builds[1:]:
        faster, not_above = {}, {}
        for wname, _, _ in WINDOWS:
            c, p = runs[(wname, label)], runs[(wname, parent)]
            faster[wname] = max(c) < min(p)
            not_above[wname] = med[(wname, label)] <= med[(wname, parent)]
            print(f"{wname:6s} {label} vs {parent}: median ratio {med[(wname, label)] / med[(wname, parent)]:.4f}; "
                  f"every run faster than every parent run: {faster[wname]}; parent spread "
                  f"{min(p):.4f}-{max(p):.4f}")
        keep = (faster["plain"] and not_above["steady"]) or (faster["steady"] and not_above["plain"])
        print(f"keep rule, {label}: {'PASS' if keep else 'FAIL'}")


if __name__ == "__main__":
    main()
