#!/usr/bin/env python3
"""Cost of PLONK public inputs (include/pbf.h "Public inputs"), one process per size:

  prove LOG_N     one proof of a 2^LOG_N-gate circuit: the plain entry (the yardstick), the _pi entry
                  with npub = 0, 2^10 and n, alternating inside each repetition (the order rotates); then the prover's
                  own marks of one _pi proof (option prover.timing), whose "public inputs" line is the
                  added INTT(n) + coset NTT(4n), beside the measured difference
  batch [K]       K (default 4096) proofs of a 2^10-gate circuit in one batched verification: the
                  plain batch entry (the yardstick), the _pi entry with npub = 0, 16 and 1024
  single LOG_N    one proof with npub = n = 2^LOG_N through the single verifiers

--yardstick-lib PATH takes the yardstick from another build of libpbf.so (the parent commit's), in
its own context; without it the yardstick is this build's plain entry. Every path has a context
of its own, so no path evicts another's proving or verification key.

Circuit and statement: the synthetic mul circuit (q_c = 0) is the q' form; the public-input
circuit has q_c[i] = pub_i on rows i < npub, which the same witness satisfies under the statement
pub. All proofs of a batch therefore share one pub (the arrays are still per proof)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pbf  # noqa: E402
from bench_prover import G2, breakdown  # noqa: E402

S = 0x5EED0005C0FFEE
CHAL = [0x1111 * (i + 3) for i in range(5)]
RND = [0x2222 * (i + 5) for i in range(9)]
K1K2 = pbf.ints_to_limbs([2, 3])


class Raw:
    """A context of a given libpbf.so (this build's, or the yardstick's)."""

    def __init__(self, path=None):
        if path:
            self.lib = ctypes.CDLL(path)
            for name, res, args in pbf.SIGNATURES:
                if hasattr(self.lib, name):
                    fn = getattr(self.lib, name)
                    fn.restype, fn.argtypes = res, args
        else:
            self.lib = pbf.load_library()
        self.h = ctypes.c_void_p()
        assert self.lib.pbf_ctx_create(0, ctypes.byref(self.h)) == 0

    def ok(self, rc):
        if rc:
            raise RuntimeError((rc, self.lib.pbf_last_error()))

    def close(self):
        self.lib.pbf_ctx_destroy(self.h)


def rand_pub(npub, seed):
    """npub canonical values (below 2^252) as limbs."""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=4 * max(npub, 1), dtype=np.int64).astype(np.uint64)
    a[3::4] &= np.uint64((1 << 60) - 1)
    return a[:4 * npub]


def circuit(n):
    sp = torch.cuda.current_stream().cuda_stream
    ctx = pbf.Context(0)
    dq = torch.empty(5 * n * 4, dtype=torch.int64, device="cuda")
    dc = torch.empty(3 * n * 2, dtype=torch.int64, device="cuda")
    dabc = torch.empty(3 * n * 4, dtype=torch.int64, device="cuda")
    ctx.plonk_synth_circuit_dev(n, 0x5EED0005, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), stream=sp)
    dsrs = torch.empty((n + 3) * 8, dtype=torch.int64, device="cuda")
    ctx.srs_create_dev(S, n + 2, dsrs.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    g2l = pbf._g2_limbs([G2, ctx.g2_bn254_mul([G2], [S])[0]])
    ctx.close()
    return sp, dq, dc, dabc, dsrs, g2l


def with_pub(dq, n, pub):
    """(q with q_c[i] = pub_i, pub on the device)."""
    d = dq.clone()
    dp = torch.from_numpy(pub.view(np.int64).copy()).cuda()
    d[16 * n:16 * n + len(pub)] = dp
    return d, dp


def report(name, ts, base=None):
    v = sorted(ts)
    med = v[len(v) // 2]
    extra = "" if base is None else f" | {1e3 * (med - base):+9.3f} ms vs yardstick"
    print(f"{name:34s} | {med * 1e3:10.3f} ms ({v[0] * 1e3:.3f} - {v[-1] * 1e3:.3f}){extra}", flush=True)
    return med


def alternate(paths, reps):
    for _, fn in paths:
        fn()  # warm-up: plans, buffers, keys
        fn()
    ts = {name: [] for name, _ in paths}
    for r in range(reps):
        # the order rotates: every path follows every other equally often, so what a path inherits
        # from its predecessor (another library's kernels, another context's working set) lands in
        # a minority of its samples, which the median ignores and the min-max shows
        k = r % len(paths)
        for name, fn in paths[k:] + paths[:k]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
    base = None
    for i, (name, _) in enumerate(paths):
        med = report(name, ts[name], base)
        base = med if i == 0 else base


def prove_fn(c, n, q, dc, abc, srs, pub, npub, sp, out, plain=False):
    pts, fs = np.zeros(72, dtype=np.uint64), np.zeros(28, dtype=np.uint64)
    out.append((pts, fs))
    ch, rn = pbf.ints_to_limbs(CHAL), pbf.ints_to_limbs(RND)
    if plain:
        return lambda: c.ok(c.lib.pbf_plonk_prove_bn254_dev(c.h, n, q.data_ptr(), dc.data_ptr(), abc.data_ptr(),
                                                            pbf._ptr(ch),
                                                            pbf._ptr(rn), pbf._ptr(K1K2), srs.data_ptr(), n + 3, 1,
                                                            pbf._ptr(pts), pbf._ptr(fs), sp))
    return lambda: c.ok(c.lib.pbf_plonk_prove_bn254_pi_dev(c.h, n, q.data_ptr(), dc.data_ptr(), abc.data_ptr(),
                                                           pub.data_ptr() if npub else None, npub, pbf._ptr(ch),
                                                           pbf._ptr(rn), pbf._ptr(K1K2), srs.data_ptr(), n + 3, 1,
                                                           pbf._ptr(pts), pbf._ptr(fs), sp))


def bench_prove(log_n, ylib, reps=10):
    n = 1 << log_n
    sp, dq, dc, dabc, dsrs, _ = circuit(n)
    print(f"# prove: n = 2^{log_n} gates, paper mode, proving key cached, {reps} repetitions, yardstick = plain entry of "
          f"{os.path.basename(ylib) if ylib else 'this build'}, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the yardstick")
    out, paths, ctxs, keep = [], [], [], []
    cy = Raw(ylib)
    ctxs.append(cy)
    paths.append(("plain entry (yardstick)", prove_fn(cy, n, dq, dc, dabc, dsrs, None, 0, sp, out, plain=True)))
    if ylib:
        c = Raw()
        ctxs.append(c)
        paths.append(("plain entry, this build", prove_fn(c, n, dq, dc, dabc, dsrs, None, 0, sp, [], plain=True)))
    pi_ctx = None
    for npub in sorted({0, min(n, 1 << 10), n}):
        c = Raw()
        ctxs.append(c)
        q, dp = with_pub(dq, n, rand_pub(npub, npub + 1))
        keep.append((q, dp))
        paths.append((f"_pi entry, npub = {npub}", prove_fn(c, n, q, dc, dabc, dsrs, dp, npub, sp, out)))
        pi_ctx = (c, paths[-1][1])
    alternate(paths, reps)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "npub = 0 differs"
    c, fn = pi_ctx
    holder = type("H", (), {"set_option": lambda self, k, v: c.ok(c.lib.pbf_ctx_set_option(
        c.h, k.encode(), None if v is None else str(v).encode()))})()
    marks = breakdown(holder, fn)
    print(f"# marks of one _pi proof, npub = {n} (stream synchronised at each mark):")
    for k, v in marks.items():
        print(f"#   {k:44s} {v:9.3f} ms")
    for c in ctxs:
        c.close()


def bench_batch(K, ylib, reps=10, log_n=10):
    n = 1 << log_n
    sp, dq, dc, dabc, dsrs, g2l = circuit(n)
    print(f"# batch: {K} proofs of a 2^{log_n}-gate circuit, verification key cached, {reps} repetitions, yardstick = "
          f"plain batch entry of {os.path.basename(ylib) if ylib else 'this build'}, {torch.cuda.get_device_name(0)}")
    print("# path | median ms (min - max) | difference of medians to the yardstick")
    rng = np.random.default_rng(5)
    ua = rand_pub(K, 77)
    ra = rand_pub(K, 78) | np.uint64(1)
    ok = ctypes.c_int(-1)
    paths, ctxs, keep = [], [], []

    def proofs_of(q, pub, npub):
        c = pbf.Context(0)
        ps = []
        for d in range(4):
            chal = [int(x) for x in rng.integers(1, 1 << 62, size=5)]
            rnd = [int(x) for x in rng.integers(1, 1 << 62, size=9)]
            pts, fs = c.plonk_prove_bn254_pi_dev(n, q.data_ptr(), dc.data_ptr(), dabc.data_ptr(),
                                                 pub.data_ptr() if npub else 0, npub, chal, rnd, dsrs.data_ptr(), n + 3,
                                                 mode=1, stream=sp)
            ps.append((pts.copy(), fs.copy(), pbf.ints_to_limbs(chal)))
        c.close()
        return [np.concatenate([ps[i % 4][j] for i in range(K)]).astype(np.uint64) for j in range(3)]

    plain = proofs_of(dq, None, 0)
    cy = Raw(ylib)
    ctxs.append(cy)

    def yard():
        cy.ok(cy.lib.pbf_plonk_verify_bn254_batch_dev(cy.h, n, dq.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                      pbf._ptr(g2l), K, pbf._ptr(plain[0]), pbf._ptr(plain[1]),
                                                      pbf._ptr(plain[2]), pbf._ptr(ua), pbf._ptr(ra), pbf._ptr(K1K2), 1,
                                                      ctypes.byref(ok), None, sp))
        assert ok.value == 1

    paths.append(("plain batch entry (yardstick)", yard))
    for npub in (0, 16, n):
        pub = rand_pub(npub, npub + 1)
        q, dp = with_pub(dq, n, pub)
        pr = plain if npub == 0 else proofs_of(q, dp, npub)
        pubs = np.tile(pub, K)
        c = Raw()
        ctxs.append(c)
        keep.append((q, dp, pr, pubs))

        def run(c=c, q=q, pr=pr, pubs=pubs, npub=npub):
            c.ok(c.lib.pbf_plonk_verify_bn254_batch_pi_dev(c.h, n, q.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                           pbf._ptr(g2l), K, pbf._ptr(pr[0]), pbf._ptr(pr[1]),
                                                           pbf._ptr(pubs) if npub else None, npub, pbf._ptr(pr[2]),
                                                           pbf._ptr(ua), pbf._ptr(ra), pbf._ptr(K1K2), 1, ctypes.byref(ok),
                                                           None, sp))
            assert ok.value == 1

        paths.append((f"_pi batch entry, npub = {npub} ({K * npub * 32 / 2**20:.1f} MiB of pub uploaded)", run))
    alternate(paths, reps)
    for c in ctxs:
        c.close()


def bench_single(log_n, reps=10):
    n = 1 << log_n
    sp, dq, dc, dabc, dsrs, g2l = circuit(n)
    print(f"# single verifier: one proof of a 2^{log_n}-gate circuit with npub = n, verification key cached, {reps} "
          f"repetitions, {torch.cuda.get_device_name(0)}")
    pub = rand_pub(n, 3)
    q, dp = with_pub(dq, n, pub)
    ch, u = pbf.ints_to_limbs(CHAL), pbf.ints_to_limbs([12345])
    ok = ctypes.c_int(-1)
    ctx = pbf.Context(0)
    plain = ctx.plonk_prove_bn254_dev(n, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), CHAL, RND, dsrs.data_ptr(), n + 3,
                                      mode=1, stream=sp)
    withpi = ctx.plonk_prove_bn254_pi_dev(n, q.data_ptr(), dc.data_ptr(), dabc.data_ptr(), dp.data_ptr(), n, CHAL, RND,
                                          dsrs.data_ptr(), n + 3, mode=1, stream=sp)
    ctx.close()
    c0, c1 = Raw(), Raw()

    def v_plain():
        c0.ok(c0.lib.pbf_plonk_verify_bn254_dev(c0.h, n, dq.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                pbf._ptr(g2l), pbf._ptr(plain[0]), pbf._ptr(plain[1]), pbf._ptr(ch),
                                                pbf._ptr(u), pbf._ptr(K1K2), 1, ctypes.byref(ok), sp))
        assert ok.value == 1

    def v_pi():
        c1.ok(c1.lib.pbf_plonk_verify_bn254_pi_dev(c1.h, n, q.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), n + 3,
                                                   pbf._ptr(g2l), pbf._ptr(withpi[0]), pbf._ptr(withpi[1]), pbf._ptr(pub),
                                                   n, pbf._ptr(ch), pbf._ptr(u), pbf._ptr(K1K2), 1, ctypes.byref(ok), sp))
        assert ok.value == 1

    alternate([("plain single verifier (yardstick)", v_plain),
               (f"_pi single verifier, npub = {n} ({n * 32 / 2**20:.0f} MiB of pub uploaded)", v_pi)], reps)
    c0.close()
    c1.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    ylib = None
    if "--yardstick-lib" in argv:
        i = argv.index("--yardstick-lib")
        ylib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if argv and argv[0] == "prove":
        bench_prove(int(argv[1]), ylib)
    elif argv and argv[0] == "batch":
        bench_batch(int(argv[1]) if len(argv) > 1 else 4096, ylib)
    elif argv and argv[0] == "single":
        bench_single(int(argv[1]))
    else:
        sys.exit(__doc__)
