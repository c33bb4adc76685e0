"""The entry points of the cell proofs are declared, bound, exported and reachable from Context,
and the header states what a caller must know (CPU only: nothing is computed)."""
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
    "pbf_kzg_cells_setup_bn254": 7,
    "pbf_kzg_cells_setup_bn254_dev": 8,
    "pbf_kzg_open_cells_bn254": 12,
    "pbf_kzg_open_cells_bn254_dev": 13,
    "pbf_kzg_verify_cells_bn254": 14,
}


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    doc = " ".join(src.split())
    assert "KZG cell proofs" in doc
    # the layout of xext, so that a caller may compute or store it
    assert "a_r[t] = srs[r + l (k-2-t)]" in doc
    assert "xext[r*2k + i] = G1-NTT_{2k, omega2^l}(a_r)[i]" in doc and "slab-major" in doc
    assert "srs_m >= n - l" in doc
    # the order of the values, and what the verifier is given on the twist
    assert "out_y[(b*k + i)*l + t] = p_b(omega^(i + k t))" in doc and "cell-major" in doc
    assert "g2 = [G2, [s^l]G2]" in doc and "pbf_g2_bn254_mul" in doc
    assert "count * l <= 2^22" in doc and "cell_idx >= k" in doc
    assert "out_y may be NULL" in doc


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
        "kzg_cells_setup": ["srs", "n", "l", "omega2"],
        "kzg_cells_setup_dev": ["d_srs", "srs_m", "omega2", "n", "l", "d_xext", "stream"],
        "kzg_open_cells": ["xext", "l", "omega2", "polys", "weights", "pitch", "with_y"],
        "kzg_open_cells_dev": ["d_xext", "n", "l", "omega2", "d_polys", "length", "pitch", "batch", "weights",
                               "d_out_y", "d_out_w", "stream"],
        "kzg_verify_cells": ["g2s", "srs", "omega", "n", "l", "entries", "rhos"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name
