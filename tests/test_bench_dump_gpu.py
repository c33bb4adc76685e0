"""bench.py as the driver runs it: a plain run prints the headline line only (nothing that takes
runs of its own), and --dump-outputs writes the last timed step's NTT output, bit-exact against
the oracle, as float64 halves."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import pbf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = pbf.GOLDILOCKS
NAMES = ("ntt_out_lo32", "ntt_out_hi32", "ntt_out_sum_lo32", "ntt_out_sum_hi32")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _halves(v):
    return (v & np.uint64(0xFFFFFFFF)).astype(np.float64), (v >> np.uint64(32)).astype(np.float64)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    log_n, B, steps, warmup = 12, 3, 2, 1
    n = 1 << log_n
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--log-n", str(log_n), "--batch", str(B),
                          "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - B * n / (line["ms_per_step"] / 1e3)) / line["value"] < 2e-3  # 4 significant digits
    assert "extra" not in line and "cpu_baseline" not in line and "traffic_detail" not in line["roofline"]
    # the last of warmup + steps steps works on buffer set (warmup + steps - 1) % BUFFER_SETS
    seed = 0x5EED0002 + (warmup + steps - 1) % 3
    a = oracle.splitmix_field(GOLD, seed, B * n).reshape(B, n)
    w = pow(7, (GOLD - 1) // n, GOLD)
    want = np.concatenate([oracle.ntt_iter(GOLD, w, a[i]) for i in range(B)]).astype(np.uint64)
    lo, hi = _halves(want)
    got = {k: np.load(tmp_path / "dump" / (k + ".npy")) for k in NAMES}
    assert all(g.dtype == np.float64 for g in got.values())
    assert np.array_equal(got["ntt_out_lo32"], lo) and np.array_equal(got["ntt_out_hi32"], hi)
    assert np.array_equal(got["ntt_out_sum_lo32"], lo.reshape(B, n).sum(axis=1))
    assert np.array_equal(got["ntt_out_sum_hi32"], hi.reshape(B, n).sum(axis=1))


@pytest.mark.gpu
def test_dump_outputs_samples_a_large_output(tmp_path):
    """Above DUMP_SAMPLE elements the dump is a fixed sample plus exact sums over runs of 2^20."""
    import torch

    b = _bench()
    n, B = 1 << 21, 2  # runs of 2^20: two per polynomial
    v = np.random.default_rng(5).integers(0, GOLD, size=B * n, dtype=np.uint64)
    d = torch.from_numpy(v.view(np.int64)).cuda()
    b.dump_outputs(str(tmp_path / "a"), d, n)
    b.dump_outputs(str(tmp_path / "b"), d, n)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in NAMES}
    for k in NAMES:
        assert np.array_equal(got[k], np.load(tmp_path / "b" / (k + ".npy"))), k
    assert sum(g.nbytes for g in got.values()) <= 64 << 20
    lo, hi = _halves(v)
    idx = np.sort(np.random.Generator(np.random.PCG64(b.DUMP_SEED)).choice(v.size, b.DUMP_SAMPLE, replace=False))
    assert got["ntt_out_lo32"].shape == (b.DUMP_SAMPLE,)
    assert np.array_equal(got["ntt_out_lo32"], lo[idx]) and np.array_equal(got["ntt_out_hi32"], hi[idx])
    sums = v.reshape(-1, 1 << 20)
    assert np.array_equal(got["ntt_out_sum_lo32"], (sums & np.uint64(0xFFFFFFFF)).sum(axis=1).astype(np.float64))
    assert np.array_equal(got["ntt_out_sum_hi32"], (sums >> np.uint64(32)).sum(axis=1).astype(np.float64))
