"""The batched PLONK verifier is declared, bound and exported (CPU only: nothing is computed)."""
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
HEADER = os.path.join(ROOT, "include", "pbf.h")
NAMES = ("pbf_plonk_verify_bn254_batch", "pbf_plonk_verify_bn254_batch_dev")


def test_header_declares_the_batch_entry_points():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    # the contract the caller must know: who chooses the weights
    doc = " ".join(src.split())
    assert "rho" in doc and "unpredictabl" in doc


def test_binding_describes_and_loads_them():
    import pbf

    sig = {n: a for n, _, a in pbf.SIGNATURES}
    assert len(sig[NAMES[0]]) == 17 and len(sig[NAMES[1]]) == 18
    lib = pbf.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_context_has_the_methods():
    import pbf

    p = inspect.signature(pbf.Context.plonk_verify_bn254_batch).parameters
    assert list(p)[1:9] == ["q", "copies", "srs", "g2s", "proofs", "chals", "us", "rhos"]
    assert p["k1k2"].default == (2, 3) and p["mode"].default == 0 and p["each"].default is False
    d = inspect.signature(pbf.Context.plonk_verify_bn254_batch_dev).parameters
    assert list(d)[1:6] == ["n", "d_q", "d_copies", "d_srs", "srs_m"] and "stream" in d and "each" in d


def test_batch_arrays_are_proof_major():
    import pbf

    proofs = [([(1, 2)] + [None] * 8, list(range(7))), ([None] * 8 + [(3, 4)], list(range(10, 17)))]
    count, pa, fa, ca, ua, ra = pbf.Context._batch_arrays(proofs, [(1, 2, 3, 4, 5), (6, 7, 8, 9, 10)], [11, 12],
                                                          [13, 1 << 200])
    assert count == 2 and pa.shape == (144,) and fa.shape == (56,) and ca.shape == (40,)
    assert pa[0] == 1 and pa[4] == 2 and pa[72 + 64] == 3 and pa[72 + 68] == 4
    assert fa[28 + 4] == 11 and ca[20] == 6 and ua[4] == 12 and ra[0] == 13 and ra[7] == 1 << 8
