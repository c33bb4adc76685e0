"""Launch-sequence check of the PLONK prover, verifiers and KZG entry points (profiles/prover_terms/).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/prover_launch_seq.py run
  python scripts/prover_launch_seq.py seq DIR/.../t_kernel_trace.csv > launches.txt
  python scripts/prover_launch_seq.py digest launches.txt > launches_digest.txt

`run` enqueues, through the library that PBF_LIB selects (default: the tree's libpbf.so), at
n = 2^10 and in modes 0 and 1: a first proof (proving key built), a second (key hit), one with
prover.pk = 0 and one with ntt256.l29 = 0; a verify with the verification key built, cached and
with verifier.vk = 0; a 4-proof verify_batch with one bad proof (so localisation runs); KZG commit,
open and verify of 2 polynomials of 2^10 coefficients; and the sharded prover on G = 2 virtual
ranks, two proofs per rank in each mode and once with prover.pk = 0. `seq` prints kernel name, grid
and workgroup size of every dispatch (scripts/ntt_launch_seq.py), per host thread: the main
thread's in dispatch order first, then the rank threads' blocks, sorted by their text, since
which rank thread dispatches first is not fixed. Two libraries launch the same kernels when the
two outputs are equal. `digest` shrinks a `seq` output to what is worth keeping: per thread the
number of dispatches and the SHA-256 of its lines, then the dispatch count per kernel name."""
import collections
import contextlib
import csv
import hashlib
import io
import os
import random
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ntt_launch_seq import seq as seq_one  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))


def seq(path):
    rows = list(csv.DictReader(open(path)))
    cols = list(rows[0].keys())
    tid = [c for c in cols if "thread" in c.lower()][0]
    disp = [c for c in cols if "dispatch_id" in c.lower()][0]
    rows.sort(key=lambda r: int(r[disp]))
    threads = []
    for r in rows:
        if r[tid] not in threads:
            threads.append(r[tid])
    blocks = []
    for t in threads:  # the main thread dispatches first
        with tempfile.NamedTemporaryFile("w", suffix=".csv", newline="") as f:
            w = csv.DictWriter(f, fieldnames=cols)
            w.writeheader()
            w.writerows(r for r in rows if r[tid] == t)
            f.flush()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                seq_one(f.name)
        blocks.append(buf.getvalue())
    for k, b in enumerate([blocks[0]] + sorted(blocks[1:])):
        print("# thread %d" % k)
        sys.stdout.write(b)


def digest(path):
    blocks = open(path).read().split("# thread ")[1:]
    names = collections.Counter()
    for b in blocks:
        head, lines = b.split("\n", 1)
        rows = lines.splitlines()
        print("thread %s: %d dispatches, sha256 %s" % (head, len(rows), hashlib.sha256(lines.encode()).hexdigest()))
        names.update(r.rsplit(" grid=", 1)[0] for r in rows)
    for name, count in sorted(names.items()):
        print("%6d  %s" % (count, name))


def run():
    import torch

    import pbf
    from multigpu import LocalComm, LocalGroup, ShardedProver

    n, s_secret = 1 << 10, 0x5EED0005C0FFEE
    sp = torch.cuda.current_stream().cuda_stream
    rng = random.Random(0x5EED)
    base = pbf.Context(0)
    dq = torch.empty(5 * n * 4, dtype=torch.int64, device="cuda")
    dc = torch.empty(3 * n * 2, dtype=torch.int64, device="cuda")
    dabc = torch.empty(3 * n * 4, dtype=torch.int64, device="cuda")
    base.plonk_synth_circuit_dev(n, 0x5EED0005, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), stream=sp)
    srs_m = 2 * n + 2
    dsrs = torch.empty(srs_m * 8, dtype=torch.int64, device="cuda")
    base.srs_create_dev(s_secret, srs_m - 1, dsrs.data_ptr(), stream=sp)
    g2s = [G2, base.g2_bn254_mul([G2], [s_secret])[0]]
    torch.cuda.synchronize()
    chal = [rng.randrange(R) for _ in range(5)]
    rnd = [rng.randrange(R) for _ in range(9)]

    def prove(c, mode):
        out = c.plonk_prove_bn254_dev(n, dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), chal, rnd, dsrs.data_ptr(),
                                      srs_m, mode=mode, stream=sp)
        torch.cuda.synchronize()
        return out

    for mode in (0, 1):
        c = pbf.Context(0)
        proof = prove(c, mode)  # key built
        assert all((a == b).all() for a, b in zip(proof, prove(c, mode)))  # key hit
        c.set_option("prover.pk", 0)
        prove(c, mode)
        c.set_option("prover.pk", None)
        c29 = pbf.Context(0, options={"ntt256.l29": 0})
        assert all((a == b).all() for a, b in zip(proof, prove(c29, mode)))
        c29.close()
        # verify: key built, cached, off
        for k in range(3):
            if k == 2:
                c.set_option("verifier.vk", 0)
            ok = c.plonk_verify_bn254_dev(n, dq.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), srs_m, g2s, proof[0],
                                          proof[1], chal, 12345, mode=mode, stream=sp)
            assert ok == (mode == 1)  # the reference's own verifier rejects its mode-0 proofs
            torch.cuda.synchronize()
        c.set_option("verifier.vk", None)
        # a batch of 4 with proof 2 spoiled: the batch fails and is localised
        bad = (proof[0], proof[1].copy())
        bad[1][0] ^= 1
        ok, each = c.plonk_verify_bn254_batch_dev(n, dq.data_ptr(), dc.data_ptr(), dsrs.data_ptr(), srs_m, g2s,
                                                  [proof, proof, bad, proof], [chal] * 4, [7, 8, 9, 10],
                                                  [rng.randrange(1, R) for _ in range(4)], mode=mode, each=True,
                                                  stream=sp)
        torch.cuda.synchronize()
        assert not ok and each == [mode == 1, mode == 1, False, mode == 1], (ok, each)
        c.close()

    # KZG: commit, open, verify of 2 polynomials of 2^10 coefficients
    c = pbf.Context(0)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    srs = base.srs_create(s_secret, n)
    commits = c.kzg_commit(srs, polys)
    z, weights = rng.randrange(R), [rng.randrange(R) for _ in range(2)]
    ys, w = c.kzg_open(srs, polys, z, weights)
    cf, yf = pbf.kzg_fold(commits, ys, weights, ctx=c)
    assert c.kzg_verify(g2s, [(cf, z, yf, w)], [rng.randrange(1, R)])
    c.close()

    # sharded, G = 2 virtual ranks: two proofs per rank in each mode, then once without the key
    def sharded(mode, options, proofs):
        G = 2
        group = LocalGroup(G)
        errs = []

        def rank_main(r):
            try:
                cr = pbf.Context(0, options=options)
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    spv = ShardedProver(cr, LocalComm(group, r), r, G, n, stream=st.cuda_stream)
                    for _ in range(proofs):
                        spv.prove(dq.data_ptr(), dc.data_ptr(), dabc.data_ptr(), chal, rnd, dsrs.data_ptr(), srs_m,
                                  mode=mode)
                st.synchronize()
                cr.close()
            except Exception as e:
                errs.append(repr(e))
                group.barrier.abort()

        ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts) and not errs, errs

    sharded(0, None, 2)
    sharded(1, None, 2)
    sharded(1, {"prover.pk": 0}, 1)
    base.close()


if __name__ == "__main__":
    {"seq": seq, "digest": digest}[sys.argv[1]](sys.argv[2]) if sys.argv[1] != "run" else run()
