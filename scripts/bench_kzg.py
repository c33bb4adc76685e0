#!/usr/bin/env python3
"""The KZG entry points on one box in one process: batch = 6 polynomials (the shape of the prover's
W_z) of len = 2^20 and 2^24 coefficients, then verification at count = 1 / 256 / 4096; REPS calls
after a warm-up each.
  commit   pbf_kzg_commit_bn254_dev (6 fixed-base MSMs)
  open     pbf_kzg_open_bn254_dev including its MSM
  verify   pbf_kzg_verify_bn254
Prints the median and min-max wall time per row. (profiles/kzg/open_ab.txt is this script's output
from when it also timed the opening's sweeps without the MSM and alternated a fused single-sweep
kernel with them: DESIGN.md 3.9.)
Usage: bench_kzg.py [log2 len ...]   (default 20 24)"""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
import torch  # noqa: E402

import pbf  # noqa: E402
from bench_prover import G2  # noqa: E402

R = pbf.BN254_R
BATCH, REPS, S = 6, 7, 0x5EED0005C0FFEE


def timed(fn, reps=REPS):
    fn()  # warm-up: buffers, the window table
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def show(name, ts, extra=""):
    v = sorted(ts)
    print(f"{name:34s} | {v[len(v) // 2] * 1e3:10.3f} ms ({v[0] * 1e3:.3f} - {v[-1] * 1e3:.3f}){extra}")
    sys.stdout.flush()
    return v[len(v) // 2]


def main(logs):
    rng = random.Random(0xC0117)
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"# batch = {BATCH}, {REPS} repetitions after a warm-up, {torch.cuda.get_device_name(0)}, "
          f"{os.path.basename(pbf.LIB_PATH)}")
    print("# path | median ms (min - max)")
    for lg in logs:
        ln = 1 << lg
        dsrs = torch.empty(ln * 8, dtype=torch.int64, device="cuda")
        ctx.srs_create_dev(S, ln - 1, dsrs.data_ptr(), stream=sp)
        polys = torch.randint(-(1 << 63), (1 << 63) - 1, (BATCH * ln, 4), dtype=torch.int64, device="cuda")
        polys[:, 3] &= (1 << 60) - 1  # canonical: below r's top limb
        torch.cuda.synchronize()
        z = rng.randrange(R)
        weights = [rng.randrange(R) for _ in range(BATCH)]

        def opn():
            return ctx.kzg_open_dev(dsrs.data_ptr(), ln, polys.data_ptr(), ln, ln, BATCH, z, weights, stream=sp)

        show(f"commit 2^{lg} x {BATCH}",
             timed(lambda: ctx.kzg_commit_dev(dsrs.data_ptr(), ln, polys.data_ptr(), ln, ln, BATCH, stream=sp)))
        show(f"open 2^{lg} x {BATCH} (with MSM)", timed(opn))
        del dsrs, polys
        ctx.release_caches()
        torch.cuda.empty_cache()
    # verification: 5 distinct small openings cycled, each entry with its own rho
    srs = ctx.srs_create(S, 17)
    g2s = [G2, ctx.g2_bn254_mul([G2], [S])[0]]
    base = []
    for _ in range(5):
        p = [rng.randrange(R) for _ in range(17)]
        zz = rng.randrange(R)
        (c,) = ctx.kzg_commit(srs, [p])
        (y,), w = ctx.kzg_open(srs, [p], zz, [1])
        base.append((c, zz, y, w))
    for count in (1, 256, 4096):
        ents = [base[i % 5] for i in range(count)]
        arrs = (pbf._g2_limbs(g2s), pbf._g1_limbs([e[0] for e in ents]), pbf.ints_to_limbs([e[1] for e in ents]),
                pbf.ints_to_limbs([e[2] for e in ents]), pbf._g1_limbs([e[3] for e in ents]),
                pbf.ints_to_limbs([rng.randrange(1, R) for _ in range(count)]))
        ok = ctypes.c_int(-1)

        def ver():
            pbf._check(ctx.lib.pbf_kzg_verify_bn254(ctx.h, pbf._ptr(arrs[0]), count, pbf._ptr(arrs[1]),
                                                    pbf._ptr(arrs[2]), pbf._ptr(arrs[3]), pbf._ptr(arrs[4]),
                                                    pbf._ptr(arrs[5]), ctypes.byref(ok)))
            assert ok.value == 1

        med = show(f"verify count = {count}", timed(ver))
        print(f"#   {med / count * 1e6:.1f} us per opening")
    ctx.close()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [20, 24])
