#!/usr/bin/env python3
"""Cost of the Fiat-Shamir transcript (include/pbf.h "Fiat-Shamir"), one process per part:

  transcript      pbf_plonk_challenges_bn254 (all host pointers: upload, kernels, download) at 4096
                  proofs with npub = 0 / 16 / 1024 and at one proof with npub = 2^20. The single-thread
                  host loop over the same __host__ Keccak-f is scripts/ubench/fs_host, run beside it.
  batch [K]       K (default 4096) proofs of a 2^10-gate circuit: pbf_plonk_verify_bn254_batch_fs_dev
                  with npub = 0 / 16 / 1024 against the plain batch entries fed the same challenges
                  (which exclude any transcript), alternating inside each repetition
  prove LOG_N     one proof of a 2^LOG_N-gate circuit: pbf_plonk_prove_bn254_fs_dev against the plain
                  entry, alternating; then the prover's own marks of one _fs proof (option
                  prover.timing), whose "fs:" lines are the added collection points

--yardstick-lib PATH takes the plain entries from another build of libpbf.so (the parent commit's),
in its own context. Every path has a context of its own."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pbf  # noqa: E402
from bench_plonk_pi import K1K2, RND, Raw, alternate, circuit, rand_pub, with_pub  # noqa: E402
from bench_prover import breakdown  # noqa: E402

P8 = pbf._p8


def digest_of(c, n, q, dc, dsrs, g2l, npub, sp):
    d = np.zeros(32, dtype=np.uint8)
    c.ok(c.lib.pbf_plonk_circuit_digest_bn254_dev(c.h, n, q.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                  pbf._ptr(g2l), pbf._ptr(K1K2), 1, npub, d.ctypes.data_as(P8), sp))
    return d


def prove_fs(c, n, q, dc, dabc, dp, npub, d, dsrs, sp, out=None, rnd=RND):
    pts, fs, ch = np.zeros(72, dtype=np.uint64), np.zeros(28, dtype=np.uint64), np.zeros(24, dtype=np.uint64)
    if out is not None:
        out.append((pts, fs, ch))
    rn = pbf.ints_to_limbs(rnd)
    return lambda: c.ok(c.lib.pbf_plonk_prove_bn254_fs_dev(c.h, n, q.data_ptr(), dc.data_ptr(), dabc.data_ptr(),
                                                           dp.data_ptr() if npub else None, npub, d.ctypes.data_as(P8),
                                                           pbf._ptr(rn), pbf._ptr(K1K2), dsrs.data_ptr(), n + 3, 1,
                                                           pbf._ptr(pts), pbf._ptr(fs), pbf._ptr(ch), sp))


def bench_transcript(reps=10):
    print(f"# transcript: pbf_plonk_challenges_bn254 (upload, kernels, download), {reps} repetitions, "
          f"{torch.cuda.get_device_name(0)}")
    print("# shape | median ms (min - max)")
    c = Raw()
    d = np.frombuffer(bytes(range(32)), dtype=np.uint8).copy()
    for count, npub in ((4096, 0), (4096, 16), (4096, 1024), (1, 1 << 20)):
        pts, fs = rand_pub(18 * count, 1), rand_pub(7 * count, 2)
        pub = rand_pub(count * npub, 3)
        chal, u, rho = (np.zeros(4 * k * count, dtype=np.uint64) for k in (5, 1, 1))

        def run():
            c.ok(c.lib.pbf_plonk_challenges_bn254(c.h, d.ctypes.data_as(P8), count, pbf._ptr(pts), pbf._ptr(fs),
                                                  pbf._ptr(pub) if npub else None, npub, pbf._ptr(chal), pbf._ptr(u),
                                                  pbf._ptr(rho)))

        run()
        run()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print(f"count {count:5d} npub {npub:8d} ({count * npub * 32 / 2**20:6.1f} MiB of pub) | "
              f"{ts[len(ts) // 2] * 1e3:9.3f} ms ({ts[0] * 1e3:.3f} - {ts[-1] * 1e3:.3f})", flush=True)
    c.close()


def bench_batch(K, ylib, reps=10, log_n=10):
    n = 1 << log_n
    sp, dq, dc, dabc, dsrs, g2l = circuit(n)
    print(f"# batch: {K} proofs of a 2^{log_n}-gate circuit, verification key cached, {reps} repetitions, yardstick = "
          f"plain batch entries of {os.path.basename(ylib) if ylib else 'this build'} fed the transcript's challenges, "
          f"{torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the first path")
    ok = ctypes.c_int(-1)
    ctxs, keep = [], []
    for npub in (0, 16, n):
        pub = rand_pub(npub, npub + 1)
        q, dp = with_pub(dq, n, pub)
        mk = Raw()
        d = digest_of(mk, n, q, dc, dsrs, g2l, npub, sp)
        made = []
        for k in range(4):  # four distinct proofs (their blinders differ), tiled to K
            prove_fs(mk, n, q, dc, dabc, dp, npub, d, dsrs, sp, made, [x + k for x in RND])()
        torch.cuda.synchronize()
        pa = np.concatenate([made[i % 4][0] for i in range(K)])
        fa = np.concatenate([made[i % 4][1] for i in range(K)])
        pubs = np.tile(pub, K)
        chal, u, rho = (np.zeros(4 * k * K, dtype=np.uint64) for k in (5, 1, 1))
        mk.ok(mk.lib.pbf_plonk_challenges_bn254(mk.h, d.ctypes.data_as(P8), K, pbf._ptr(pa), pbf._ptr(fa),
                                                pbf._ptr(pubs) if npub else None, npub, pbf._ptr(chal), pbf._ptr(u),
                                                pbf._ptr(rho)))
        mk.close()
        cy, c = Raw(ylib), Raw()
        ctxs += [cy, c]
        keep.append((q, dp, pa, fa, pubs, chal, u, rho))

        def yard(cy=cy, q=q, pa=pa, fa=fa, pubs=pubs, npub=npub, chal=chal, u=u, rho=rho):
            cy.ok(cy.lib.pbf_plonk_verify_bn254_batch_pi_dev(cy.h, n, q.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                             pbf._ptr(g2l), K, pbf._ptr(pa), pbf._ptr(fa),
                                                             pbf._ptr(pubs) if npub else None, npub, pbf._ptr(chal),
                                                             pbf._ptr(u), pbf._ptr(rho), pbf._ptr(K1K2), 1,
                                                             ctypes.byref(ok), None, sp))
            assert ok.value == 1

        def run(c=c, q=q, pa=pa, fa=fa, pubs=pubs, npub=npub):
            c.ok(c.lib.pbf_plonk_verify_bn254_batch_fs_dev(c.h, n, q.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                           pbf._ptr(g2l), K, pbf._ptr(pa), pbf._ptr(fa),
                                                           pbf._ptr(pubs) if npub else None, npub, pbf._ptr(K1K2), 1,
                                                           ctypes.byref(ok), None, sp))
            assert ok.value == 1

        alternate([(f"plain batch, challenges given, npub = {npub}", yard), (f"batch_fs, npub = {npub}", run)], reps)
    for c in ctxs:
        c.close()


def bench_prove(log_n, ylib, reps=10):
    n = 1 << log_n
    sp, dq, dc, dabc, dsrs, g2l = circuit(n)
    print(f"# prove: n = 2^{log_n} gates, paper mode, proving key cached, {reps} repetitions, yardstick = plain entry of "
          f"{os.path.basename(ylib) if ylib else 'this build'}, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the yardstick")
    from bench_plonk_pi import prove_fn

    paths, ctxs, keep = [], [], []
    cy = Raw(ylib)
    ctxs.append(cy)
    paths.append(("plain entry (yardstick)", prove_fn(cy, n, dq, dc, dabc, dsrs, None, 0, sp, [], plain=True)))
    if ylib:
        c = Raw()
        ctxs.append(c)
        paths.append(("plain entry, this build", prove_fn(c, n, dq, dc, dabc, dsrs, None, 0, sp, [], plain=True)))
    last = None
    for npub in sorted({0, min(n, 1 << 10)}):
        c = Raw()
        ctxs.append(c)
        q, dp = with_pub(dq, n, rand_pub(npub, npub + 1))
        d = digest_of(c, n, q, dc, dsrs, g2l, npub, sp)
        keep.append((q, dp, d))
        paths.append((f"_fs entry, npub = {npub}", prove_fs(c, n, q, dc, dabc, dp, npub, d, dsrs, sp)))
        last = (c, paths[-1][1], npub)
    alternate(paths, reps)
    c, fn, npub = last
    holder = type("H", (), {"set_option": lambda self, k, v: c.ok(c.lib.pbf_ctx_set_option(
        c.h, k.encode(), None if v is None else str(v).encode()))})()
    marks = breakdown(holder, fn)
    print(f"# marks of one _fs proof, npub = {npub} (stream synchronised at each mark):")
    for k, v in marks.items():
        print(f"#   {k:44s} {v:9.3f} ms")
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    ylib = None
    if "--yardstick-lib" in argv:
        i = argv.index("--yardstick-lib")
        ylib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if argv and argv[0] == "transcript":
        bench_transcript()
    elif argv and argv[0] == "batch":
        bench_batch(int(argv[1]) if len(argv) > 1 else 4096, ylib)
    elif argv and argv[0] == "prove":
        bench_prove(int(argv[1]), ylib)
    else:
        sys.exit(__doc__)
