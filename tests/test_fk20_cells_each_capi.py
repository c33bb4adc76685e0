"""The entry points of the batched G1 NTT and of the cell proofs of each polynomial are declared,
bound, exported and reachable from Context, and the header states what a caller must know (CPU
only: nothing is computed)."""
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
HEADER = os.path.join(ROOT, "include", "pbf.h")
# name -> number of C arguments
NAMES = {
    "pbf_ntt_g1_bn254_batch": 7,
    "pbf_ntt_g1_bn254_batch_dev": 8,
    "pbf_kzg_open_cells_each_bn254": 11,
    "pbf_kzg_open_cells_each_bn254_dev": 12,
}


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    doc = " ".join(src.split())
    # the layout and the limits of the batched transform
    assert "transform b at in + 8*b*n" in doc
    assert "n * batch <= 2^28" in doc
    # the layout and the limits of the proofs of each polynomial, and what the context keeps
    assert "out_w[b*k + i] = W_i of p_b" in doc and "polynomial-major" in doc
    assert "batch * n <= 2^24" in doc
    assert "batch x (2n + 2k) x 128 B" in doc
    # the setup runs on the batch
    assert "The l transforms run one after another" not in doc


def test_binding_describes_and_loads_them():
    import pbf

    sig = {n: (r, a) for n, r, a in pbf.SIGNATURES}
    lib = pbf.load_library()
    for name, nargs in NAMES.items():
        assert name in sig, name
        assert len(sig[name][1]) == nargs, name
        assert hasattr(lib, name), name


def test_exported_with_c_linkage():
    import pbf

    out = subprocess.run(["nm", "-D", "--defined-only", pbf.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (pbf_[a-z0-9_]+)", out.stdout))
    assert set(NAMES) <= exported, sorted(set(NAMES) - exported)


def test_context_has_the_methods():
    import pbf

    want = {
        "ntt_g1_batch": ["omega", "points", "n", "inverse"],
        "ntt_g1_batch_dev": ["omega", "d_in", "d_out", "n", "batch", "inverse", "stream"],
        "kzg_open_cells_each": ["xext", "l", "omega2", "polys", "pitch", "with_y"],
        "kzg_open_cells_each_dev": ["d_xext", "n", "l", "omega2", "d_polys", "length", "pitch", "batch", "d_out_y",
                                    "d_out_w", "stream"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name
