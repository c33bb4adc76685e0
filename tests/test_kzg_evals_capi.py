"""The entry points of KZG in evaluation form are declared, bound, exported and reachable from
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
    "pbf_ntt_g1_bn254": 6,
    "pbf_ntt_g1_bn254_dev": 7,
    "pbf_kzg_open_evals_bn254": 11,
    "pbf_kzg_open_evals_bn254_dev": 12,
}


def test_header_declares_the_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    doc = " ".join(src.split())
    assert "KZG in evaluation form" in doc
    # the in-H behaviour: no value of z fails, and how z = omega^k is handled
    assert "z inside H is no failing case" in doc and "q_k = -omega^-k" in doc
    # the Lagrange SRS is the inverse G1 NTT, and commit from evaluations is the existing commit
    assert "lsrs = the inverse G1 NTT of srs[0 .. n)" in doc
    assert "Commit from evaluations needs no entry point of its own" in doc
    # one window table per context
    assert "One window table per context" in doc and "two contexts" in doc
    assert "g1ntt.tile_log" in doc


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
        "ntt_g1": ["omega", "points", "inverse"],
        "ntt_g1_dev": ["omega", "d_in", "d_out", "n", "inverse", "stream"],
        "srs_lagrange": ["srs", "n", "omega"],
        "kzg_open_evals": ["lsrs", "omega", "evals", "z", "weights", "pitch"],
        "kzg_open_evals_dev": ["d_lsrs", "n", "omega", "d_evals", "pitch", "batch", "z", "weights", "stream"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(pbf.Context, name)).parameters)[1:] == params, name


def test_g1_ntt_option_is_accepted_by_name():
    capi = open(os.path.join(ROOT, "plonk-by-fingers_amd", "csrc", "capi.hip")).read()
    known = re.search(r"known\[\] = \{(.*?)\};", capi, flags=re.S).group(1)
    assert '"g1ntt.tile_log"' in known
