#!/usr/bin/env python3
"""Batched PLONK verification against K sequential single verifications, on one box in one
process: a 2^10-gate circuit with its verification key cached, K entries built from 4 distinct
proofs (each entry its own u and rho). Per K the two paths alternate, REPS times after a warm-up:
  (a) K calls of pbf_plonk_verify_bn254_dev                 (the baseline)
  (b) one call of pbf_plonk_verify_bn254_batch_dev
  (c) (b) with one bad proof and ok_each requested           (the cost of the halving)
Prints the median and min-max wall time per path, per-proof time and proofs/s.
Usage: bench_verify_batch.py [--batch-only] [K ...]   (default 1 16 256 4096; --batch-only skips
(a), for comparing builds of the batch path through PBF_LIB)"""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pbf  # noqa: E402
from bench_prover import G2  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
LOG_N, DISTINCT, REPS = 10, 4, 5


def main(ks, batch_only=False):
    n = 1 << LOG_N
    rng = random.Random(0xBA7C4)
    ctx = pbf.Context(0)
    sp = torch.cuda.current_stream().cuda_stream
    dq = torch.empty(5 * n * 4, dtype=torch.int64, device="cuda")
    dc = torch.empty(3 * n * 2, dtype=torch.int64, device="cuda")
    dabc = torch.empty(3 * n * 4, dtype=torch.int64, device="cuda")
    ctx.plonk_synth_circuit_dev(n, 0x5EED0005, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), stream=sp)
    srs_m, s = n + 3, 0x5EED0005C0FFEE
    dsrs = torch.empty(srs_m * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(s, srs_m - 1, dsrs.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    g2l = pbf._g2_limbs([G2, ctx.g2_bn254_mul([G2], [s])[0]])
    k1k2 = pbf.ints_to_limbs([2, 3])
    proofs = []
    for _ in range(DISTINCT):
        chal = [rng.randrange(R) for _ in range(5)]
        rnd = [rng.randrange(R) for _ in range(9)]
        pts, fs = ctx.plonk_prove_bn254_dev(n, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), chal, rnd,
                                            dsrs.data_ptr(), srs_m, mode=1, stream=sp)
        proofs.append((pts.copy(), fs.copy(), pbf.ints_to_limbs(chal)))
    args = (ctx.h, n, dq.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), srs_m, pbf._ptr(g2l))
    ok = ctypes.c_int(-1)
    print(f"# n = 2^{LOG_N} gates, verification key cached, {DISTINCT} distinct proofs, {REPS} repetitions, "
          f"{torch.cuda.get_device_name(0)}")
    print("# path: K | median ms (min - max) | us per proof | proofs/s")
    for K in ks:
        pa = np.concatenate([proofs[i % DISTINCT][0] for i in range(K)]).astype(np.uint64)
        fa = np.concatenate([proofs[i % DISTINCT][1] for i in range(K)]).astype(np.uint64)
        ca = np.concatenate([proofs[i % DISTINCT][2] for i in range(K)]).astype(np.uint64)
        ua = pbf.ints_to_limbs([rng.randrange(R) for _ in range(K)])
        ra = pbf.ints_to_limbs([rng.randrange(1, R) for _ in range(K)])
        fbad = fa.copy()
        fbad[28 * (K // 3)] ^= 1  # a_z of one proof
        each = (ctypes.c_int * K)()
        ptr = [[pbf._ptr(a[w * i:w * i + w]) for a, w in ((pa, 72), (fa, 28), (ca, 20), (ua, 4))] for i in range(K)]

        def single():
            good = 0
            for p in ptr:
                pbf._check(ctx.lib.pbf_plonk_verify_bn254_dev(*args, p[0], p[1], p[2], p[3], pbf._ptr(k1k2), 1,
                                                              ctypes.byref(ok), sp))
                good += ok.value
            return good == K

        def batch(fields=fa, oe=None):
            pbf._check(ctx.lib.pbf_plonk_verify_bn254_batch_dev(*args, K, pbf._ptr(pa), pbf._ptr(fields),
                                                                pbf._ptr(ca), pbf._ptr(ua), pbf._ptr(ra),
                                                                pbf._ptr(k1k2), 1, ctypes.byref(ok), oe, sp))
            return ok.value == 1

        def bad():
            r = batch(fbad, each)
            return (not r) and [i for i in range(K) if not each[i]] == [K // 3]

        paths = (("a single x K", single), ("b batch", batch), ("c batch, 1 bad, ok_each", bad))[batch_only:]
        for _, fn in paths:  # warm-up: buffers, the verification key, the pairing lines
            assert fn()
        ts = {name: [] for name, _ in paths}
        for _ in range(REPS):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                good = fn()
                ts[name].append(time.perf_counter() - t0)
                assert good, name
        for name, _ in paths:
            v = sorted(ts[name])
            med = v[len(v) // 2]
            print(f"{name:26s} K={K:5d} | {med * 1e3:10.3f} ms ({v[0] * 1e3:.3f} - {v[-1] * 1e3:.3f}) | "
                  f"{med / K * 1e6:9.1f} us | {K / med:10.0f}")
        sys.stdout.flush()
    ctx.close()


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--batch-only"]
    main([int(a) for a in argv] or [1, 16, 256, 4096], batch_only=len(argv) != len(sys.argv) - 1)
