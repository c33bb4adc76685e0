"""The entry points of the recovery from cells are declared, bound, exported and reachable from
Context, and the header states what a caller must know (CPU only: nothing is computed)."""
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
    "pbf_kzg_recover_cells_bn254": 13,
    "pbf_kzg_recover_cells_bn254_dev": 14,
}


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    doc = " ".join(re.sub(r"\n \*", "\n", src).split())
    assert "Recovery from cells" in doc
    # the input layout and what makes a call legal
    assert "cells[(b*count + j)*l + t]" in doc and "cell-major" in doc
    assert "count * l >= len" in doc
    assert "n/l <= 2^16" in doc
    assert "distinct" in doc
    # what consistent means, and where the proofs come from
    assert "consistent[b] = 1 exactly when every coefficient of R_b from len on is zero" in doc
    assert "With count*l == len every input is consistent" in doc
    assert "pbf_kzg_open_cells_bn254_dev on d_out_polys gives every cell's proof" in doc
    assert "out_y (may be NULL" in doc


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
        "kzg_recover_cells": ["omega", "n", "l", "length", "cell_idx", "cells", "pitch", "with_y"],
        "kzg_recover_cells_dev": ["omega", "n", "l", "length", "cell_idx", "d_cells", "batch", "d_out_polys", "pitch",
                                  "d_out_y", "d_consistent", "stream"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name
