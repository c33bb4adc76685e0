"""Launch-sequence check of the 64-bit NTT launcher (profiles/ntt_launcher/).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/ntt_launch_seq.py run
  python scripts/ntt_launch_seq.py seq DIR/.../t_kernel_trace.csv > launches.txt

`run` enqueues, through the library that PBF_LIB selects (default: the tree's libpbf.so), every
two-pass Goldilocks plan of radices 2^6 .. 2^10 with both roots, "10,10" at 2^20 x 32, the 2^24 x 2
default plan, "12,12" at 2^24 and one Mod32 transform, each forward, inverse, coset forward and
coset inverse. `seq` prints kernel name, grid and workgroup size of every dispatch of a trace in
dispatch order. Two libraries launch the same kernels when the two outputs are equal."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))


def seq(path):
    rows = list(csv.DictReader(open(path)))
    cols = list(rows[0].keys())
    pick = lambda *w: sorted(c for c in cols if all(x in c.lower() for x in w))
    name, disp = pick("kernel_name")[0], pick("dispatch_id")[0]
    grid, wg = pick("grid"), pick("workgroup")
    assert len(grid) == 3 and len(wg) == 3, cols
    rows.sort(key=lambda r: int(r[disp]))
    for r in rows:
        print("%s grid=%s wg=%s" % (r[name], ",".join(r[c] for c in grid), ",".join(r[c] for c in wg)))


def run():
    import torch

    import pbf

    GOLD, Q32 = pbf.GOLDILOCKS, 3221225473
    root = lambda m, n: pow(7 if m == GOLD else 5, (m - 1) // n, m)

    def one(opts, logn, batch, modes, m=GOLD, inverse_root=False):
        n = 1 << logn
        w = root(m, n)
        w = pow(w, m - 2, m) if inverse_root else w
        c = pbf.Context(0, options=opts)
        d_in = torch.zeros(batch * n, dtype=torch.int64, device="cuda")
        d_out = torch.empty_like(d_in)
        s = torch.cuda.current_stream().cuda_stream
        for inverse, coset in modes:
            if coset:
                in_len = n if inverse else n // 4 + 3
                c.ntt_coset_batch_dev(m, w, 7, d_in.data_ptr(), in_len, d_out.data_ptr(), n, batch, inverse=inverse,
                                      stream=s)
            else:
                c.ntt_batch_dev(m, w, d_in.data_ptr(), d_out.data_ptr(), n, batch, inverse=inverse, stream=s)
            torch.cuda.synchronize()
        c.close()

    ALL = [(False, False), (True, False), (False, True), (True, True)]
    for passes in ["6,7", "7,6", "6,8", "8,6", "6,9", "9,6", "6,10", "10,6"]:
        for ir in (False, True):
            one({"ntt.passes": passes}, sum(int(x) for x in passes.split(",")), 2, ALL, inverse_root=ir)
    one({"ntt.passes": "10,10"}, 20, 32, ALL)
    one({}, 24, 2, ALL)
    one({}, 24, 2, [(False, True), (True, True)], inverse_root=True)
    one({"ntt.passes": "12,12"}, 24, 2, [(False, False), (True, False)])
    one({}, 16, 2, ALL, m=Q32)


if __name__ == "__main__":
    seq(sys.argv[2]) if sys.argv[1] == "seq" else run()
