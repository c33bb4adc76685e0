#!/usr/bin/env python3
"""Every KZG entry point once at a small shape (n = 64, cells of 8, batch 11, len 61 at pitch 66),
for comparing two builds of the library launch by launch: open; open from evaluations with z
outside and inside H; the FK20 and cell setups; open_all and open_cells on the device with pitch >
len, and their host forms; both batched verifiers; recovery with out_y. Prints a digest of every
result. Under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/kzg_units_calls.py`
the launches land in DIR, and scripts/kzg_units_launches.py DIR lists them. PBF_LIB selects the build.
profiles/kzg_units/ holds the lists of the split of kzg.hip into units and of its parent."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bn254 as F  # noqa: E402
import bn254_pairing as B  # noqa: E402
import pbf  # noqa: E402

R = F.R
S = 0x1D0C5A11E5EED5A17ED5EC2E7000000000000000000000000000000C0FFEE % R
n, l, batch, ln, pitch = 64, 8, 11, 61, 66
k = n // l
omega2 = F.root_of_unity(2 * n)
omega = omega2 * omega2 % R
rng = random.Random(20)
ctx = pbf.Context(0)
results = []

srs = ctx.srs_create(S, n)
polys = [[rng.randrange(R) for _ in range(ln)] for _ in range(batch)]
weights = [rng.randrange(R) for _ in range(batch)]
z = rng.randrange(R)
g2 = lambda e: [B.G2_GEN, ctx.g2_bn254_mul([B.G2_GEN], [pow(S, e, R)])[0]]  # noqa: E731
g2s, g2l = g2(1), g2(l)
commits = ctx.kzg_commit(srs, polys)
lsrs = ctx.ntt_g1(omega, srs[:n], inverse=True)
evals = [[F.poly_eval(p, pow(omega, i, R)) for i in range(n)] for p in polys]
torch.cuda.synchronize()
print("MARK begin", flush=True)

# open at batch 11
o = ctx.kzg_open(srs, polys, z, weights)
results.append(o)
# open from evaluations, z outside H and inside H
results.append(ctx.kzg_open_evals(lsrs, omega, evals, z, weights))
results.append(ctx.kzg_open_evals(lsrs, omega, evals, pow(omega, 5, R), weights))
assert results[1] == results[0]

# setups, open_all and open_cells on the device, pitch > len
d_srs = torch.empty(8 * (n + 1), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
ctx.srs_create_dev(S, n, d_srs.data_ptr())
x20 = torch.empty(16 * n, dtype=torch.int64, device="cuda")
xc = torch.empty(16 * n, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
ctx.kzg_fk20_setup_dev(d_srs.data_ptr(), n + 1, omega2, n, x20.data_ptr())
ctx.kzg_cells_setup_dev(d_srs.data_ptr(), n + 1, omega2, n, l, xc.data_ptr())
a = F.random_limbs(batch * pitch, 5)
for b, p in enumerate(polys):
    a[4 * b * pitch:4 * (b * pitch + ln)] = F.ints_to_limbs(p)
d_p = torch.from_numpy(a.view(np.int64)).cuda()
outs = [torch.zeros(sz, dtype=torch.int64, device="cuda") for sz in (4 * batch * n, 8 * n, 4 * batch * n, 8 * k)]
torch.cuda.synchronize()
ctx.kzg_open_all_dev(x20.data_ptr(), n, omega2, d_p.data_ptr(), ln, pitch, batch, weights, outs[0].data_ptr(),
                     outs[1].data_ptr())
ctx.kzg_open_cells_dev(xc.data_ptr(), n, l, omega2, d_p.data_ptr(), ln, pitch, batch, weights, outs[2].data_ptr(),
                       outs[3].data_ptr())
torch.cuda.synchronize()
results += [t.cpu().numpy().tobytes() for t in outs + [x20, xc]]
# the host forms of the same
xh = ctx.kzg_cells_setup(srs[:n - l], n, l, omega2)
results.append(ctx.kzg_fk20_setup(srs[:n - 1], n, omega2))
results.append(ctx.kzg_open_all(results[-1], omega2, polys, weights))
cells = ctx.kzg_open_cells(xh, l, omega2, polys, weights)
results.append(cells)

# both verifiers
ents = []
for b in range(3):
    (y,), w = ctx.kzg_open(srs, [polys[b]], z + b, [1])
    ents.append((commits[b], z + b, y, w))
ok = ctx.kzg_verify(g2s, ents, [rng.randrange(1, R) for _ in ents])
assert ok is True
cys, cws = ctx.kzg_open_cells(xh, l, omega2, [polys[0]], [1])
cents = [(commits[0], i, cys[0][i], cws[i]) for i in (0, 3, 7, 3)]
okc = ctx.kzg_verify_cells(g2l, srs[:l], omega, n, l, cents, [rng.randrange(1, R) for _ in cents])
assert okc is True
bad = list(cents)
bad[1] = (commits[0], 3, [(v + 1) % R for v in cys[0][3]], cws[3])
assert ctx.kzg_verify_cells(g2l, srs[:l], omega, n, l, bad, [3, 4, 5, 6]) is False
results += [ok, okc]

# recovery with out_y: polynomials of 40 coefficients from 5 of the 8 cells
short = [p[:40] for p in polys[:2]]
sy, _ = ctx.kzg_open_cells(xh, l, omega2, short, [1, 1])
idx = [0, 2, 3, 5, 7]
rec = ctx.kzg_recover_cells(omega, n, l, 40, idx, [[sy[b][i] for i in idx] for b in range(2)])
assert [list(p) for p in rec[0]] == short and list(rec[2]) == [1, 1], rec[2]
results.append((str(rec[0]), str(rec[1]), str(list(rec[2]))))
torch.cuda.synchronize()
print("MARK end", flush=True)
ctx.close()
print("digest", hashlib.sha256(repr(results).encode()).hexdigest())
