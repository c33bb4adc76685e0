"""The multi-point KZG entry points are declared, bound, exported and reachable from Context
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
    "pbf_kzg_open_multi_bn254": 13,
    "pbf_kzg_open_multi_bn254_dev": 14,
    "pbf_kzg_open_multi_finish_bn254": 13,
    "pbf_kzg_open_multi_finish_bn254_dev": 14,
    "pbf_kzg_verify_multi_bn254": 15,
}


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    # the section follows "KZG commitments" and states the contract the caller must know
    assert src.index("/* ---- KZG commitments over BN254") < src.index("/* ---- Multi-point KZG openings") \
        < src.index("/* ---- KZG in evaluation form")
    doc = " ".join(src[src.index("/* ---- Multi-point KZG openings"):src.index("/* ---- KZG in evaluation form")].split())
    # who chooses rho, in the words of the KZG section
    assert "choosing the weights rho unpredictably and AFTER seeing the openings" in doc
    assert "the library reads none" in doc
    # the order of the challenges, and that the library derives none
    assert "The library derives no challenge" in doc
    assert "gamma must be derived AFTER the commitments and the evaluations y, and z AFTER W" in doc
    assert "no failing case" in doc
    assert "1 <= npts <= 32" in doc and "count * batch > 2^20" in doc
    assert "not canonical or not on the curve gives *ok = 0" in doc


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

    dev = ["d_srs", "srs_m", "d_polys", "length", "pitch", "batch"]
    want = {
        "kzg_open_multi": ["srs", "polys", "pts", "sets", "gamma", "pitch"],
        "kzg_open_multi_dev": dev + ["pts", "sets", "gamma", "stream"],
        "kzg_open_multi_finish": ["srs", "polys", "pts", "sets", "gamma", "z", "pitch"],
        "kzg_open_multi_finish_dev": dev + ["pts", "sets", "gamma", "z", "stream"],
        "kzg_verify_multi": ["g2s", "sets", "openings", "rhos"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name


def test_the_unit_is_built_and_reported():
    mk = open(os.path.join(ROOT, "plonk-by-fingers_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bkzg_multi\.hip\b", mk, flags=re.M)
    assert re.search(r"^RES_kzg_multi :=.*\bkzg_multi\b", mk, flags=re.M)
