#!/usr/bin/env python
"""Fused coset NTT / low-degree extension against the compositions a caller could write
without it. Goldilocks, shift 7, HIP events, one process:

  2^20 x 32, in_len = n   plain NTT | fused coset NTT | per-polynomial pointwise scale by a
                          device power table (pbf_pointwise_mul_u64_dev) + plain NTT
  2^18 -> 2^20 x 32       fused LDE | memset + strided copy + pointwise scale + plain NTT
                          | memset + pointwise scale straight into the padded buffer + plain NTT
  2^24 x 2, in_len = n    as the first shape

Every variant of a shape is warmed up (--warmup steps), then the variants alternate --rounds
times, each round timing --steps steps between two events; consecutive steps rotate over three
input / output sets as bench.py does. Before timing, the fused and composed outputs of the same
seeded input are compared bit for bit. One JSON line per shape: per variant the median, min and
max ms per step over the rounds.

  python scripts/bench_coset.py [--steps 20] [--warmup 20] [--rounds 5] [--shapes 20,lde,24]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))

import torch  # noqa: E402

import pbf  # noqa: E402

GOLD = pbf.GOLDILOCKS
SHIFT = 7
SETS = 3


def root_of_unity(n):
    return pow(7, (GOLD - 1) // n, GOLD)


def power_table(ctx, s, n, sp):
    """t[i] = s^i on the device, by doubling: t[f .. 2f) = t[0 .. f) * s^f"""
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    t[0] = 1
    f = 1
    while f < n:
        c = pow(s, f, GOLD)
        const = torch.full((f,), c - (1 << 64) if c >= 1 << 63 else c, dtype=torch.int64, device="cuda")
        ctx.pointwise_mul_dev(GOLD, t.data_ptr(), const.data_ptr(), t.data_ptr() + 8 * f, f, stream=sp)
        f *= 2
    torch.cuda.synchronize()
    return t


def run_shape(ctx, name, log_n, in_len, B, args, sp, stream):
    n = 1 << log_n
    w = root_of_unity(n)
    tab = power_table(ctx, SHIFT, in_len, sp)
    ins, outs = [], []
    for i in range(SETS):
        d = torch.empty(B * in_len, dtype=torch.int64, device="cuda")
        ctx.fill_random_dev(GOLD, 0x5EED0002 + i, d.data_ptr(), B * in_len, stream=sp)
        ins.append(d)
        outs.append(torch.empty(B * n, dtype=torch.int64, device="cuda"))

    def plain(i, o):
        ctx.ntt_batch_dev(GOLD, w, i.data_ptr(), o.data_ptr(), n, B, stream=sp)

    def fused(i, o):
        ctx.ntt_coset_batch_dev(GOLD, w, SHIFT, i.data_ptr(), in_len, o.data_ptr(), n, B, stream=sp)

    def scale_into(src, src_pitch, o):
        # polynomial b: o[b*n + j] = src[b*src_pitch + j] * 7^j, j < in_len (one shared table)
        for b in range(B):
            ctx.pointwise_mul_dev(GOLD, src.data_ptr() + 8 * b * src_pitch, tab.data_ptr(), o.data_ptr() + 8 * b * n,
                                  in_len, stream=sp)

    def composed(i, o):  # scale (and place) with the pointwise product, transform in place
        if in_len < n:
            o.zero_()
        scale_into(i, in_len, o)
        ctx.ntt_batch_dev(GOLD, w, o.data_ptr(), o.data_ptr(), n, B, stream=sp)

    def composed4(i, o):  # memset, strided copy, scale in place, transform in place
        o.zero_()
        o.view(B, n)[:, :in_len].copy_(i.view(B, in_len))
        scale_into(o, n, o)
        ctx.ntt_batch_dev(GOLD, w, o.data_ptr(), o.data_ptr(), n, B, stream=sp)

    variants = [("fused", fused), ("composed", composed)]
    if in_len == n:
        variants.insert(0, ("plain", plain))
    else:
        variants.append(("composed_memset_copy_scale", composed4))

    # correctness first: fused == composed on the same input
    check = torch.empty_like(outs[0])
    fused(ins[0], outs[0])
    for vname, fn in variants:
        if vname.startswith("composed"):
            fn(ins[0], check)
            torch.cuda.synchronize()
            if not torch.equal(check, outs[0]):
                raise SystemExit(f"{name}: fused and {vname} outputs differ")
    del check

    k = [0]

    def steps(fn, count):
        for _ in range(count):
            fn(ins[k[0] % SETS], outs[k[0] % SETS])
            k[0] += 1

    for _, fn in variants:
        steps(fn, args.warmup)
    torch.cuda.synchronize()
    ms = {vname: [] for vname, _ in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for vname, fn in variants:
            e0.record(stream)
            steps(fn, args.steps)
            e1.record(stream)
            torch.cuda.synchronize()
            ms[vname].append(e0.elapsed_time(e1) / args.steps)
    res = {"shape": name, "log_n": log_n, "in_len": in_len, "batch": B, "steps": args.steps, "rounds": args.rounds,
           "outputs_equal": True}
    for vname, v in ms.items():
        res[vname] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                      "max_ms": round(max(v), 5), "rounds_ms": [round(x, 5) for x in v]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="20,lde,24")
    args = ap.parse_args()
    ctx = pbf.Context(0)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for s in args.shapes.split(","):
        if s == "20":
            run_shape(ctx, "2^20 x 32", 20, 1 << 20, 32, args, sp, stream)
        elif s == "lde":
            run_shape(ctx, "2^18 -> 2^20 x 32", 20, 1 << 18, 32, args, sp, stream)
        elif s == "24":
            run_shape(ctx, "2^24 x 2", 24, 1 << 24, 2, args, sp, stream)
        else:
            raise SystemExit(f"unknown shape {s}")
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
