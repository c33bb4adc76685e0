"""The KZG commitment entry points are declared, bound, exported and reachable from Context
(CPU only: nothing is computed)."""
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
    "pbf_poly_eval_fr256": 6,
    "pbf_kzg_commit_bn254": 8,
    "pbf_kzg_commit_bn254_dev": 9,
    "pbf_kzg_open_bn254": 11,
    "pbf_kzg_open_bn254_dev": 12,
    "pbf_kzg_verify_bn254": 9,
}


def test_header_declares_the_kzg_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    # the contract the caller must know: who chooses the weights, and that opening cannot fail
    doc = " ".join(src.split())
    assert "AFTER seeing the openings" in doc and "unpredictabl" in doc
    assert "no failing case" in doc


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
        "poly_eval_fr": ["coeffs", "xs"],
        "kzg_commit": ["srs", "polys", "pitch"],
        "kzg_commit_dev": ["d_srs", "srs_m", "d_polys", "length", "pitch", "batch", "stream"],
        "kzg_open": ["srs", "polys", "z", "weights", "pitch"],
        "kzg_open_dev": ["d_srs", "srs_m", "d_polys", "length", "pitch", "batch", "z", "weights", "stream"],
        "kzg_verify": ["g2s", "entries", "rhos"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name
    assert list(inspect.signature(pbf.kzg_fold).parameters)[:3] == ["commits", "ys", "weights"]


def test_poly_limbs_respects_the_pitch():
    import pbf

    a, ln, pitch, batch = pbf.Context._poly_limbs([[1, 2, 3], [4, 5, 1 << 64]], 5)
    assert (ln, pitch, batch) == (3, 5, 2) and a.shape == (40,)
    assert a[0] == 1 and a[8] == 3 and a[12] == 0 and a[20] == 4 and a[28] == 0 and a[29] == 1
    a, ln, pitch, batch = pbf.Context._poly_limbs([[7]], None)
    assert (ln, pitch, batch) == (1, 1, 1) and list(a) == [7, 0, 0, 0]
