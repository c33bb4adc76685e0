"""The public-input entry points are declared, bound and exported (CPU only: nothing is computed)."""
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "plonk-by-fingers_amd"))
HEADER = os.path.join(ROOT, "include", "pbf.h")
# name -> number of C arguments: the plain entry's plus pub and npub
NAMES = {"pbf_plonk_prove_bn254_pi": 15, "pbf_plonk_prove_bn254_pi_dev": 16, "pbf_plonk_verify_bn254_pi": 16,
         "pbf_plonk_verify_bn254_pi_dev": 17, "pbf_plonk_verify_bn254_batch_pi": 19,
         "pbf_plonk_verify_bn254_batch_pi_dev": 20}


def test_header_declares_the_entry_points_and_their_contract():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert "size_t npub" in args and any(a.endswith("pub") and a.startswith("const uint64_t*") for a in args)
        plain = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name.replace("_pi", ""), code)
        assert len(plain.group(1).split(",")) == nargs - 2, name
    doc = " ".join(src.split())
    for must in ("npub = 0", "before anything is enqueued", "absorb pub before beta", "never a reason for ok = 0",
                 "sharded and _multi provers take no public inputs", "q_c slot is never written"):
        assert must in " ".join(doc.replace("*", " ").split()), must


def test_binding_describes_and_loads_them():
    import pbf

    sig = {n: a for n, _, a in pbf.SIGNATURES}
    lib = pbf.load_library()
    for name, nargs in NAMES.items():
        assert len(sig[name]) == nargs, name
        assert hasattr(lib, name), name


def test_context_has_the_methods():
    import pbf

    p = inspect.signature(pbf.Context.plonk_prove_bn254_pi).parameters
    assert list(p)[1:8] == ["q", "copies", "abc", "pub", "chal", "rnd", "srs"]
    assert p["k1k2"].default == (2, 3) and p["mode"].default == 0 and p["npub"].default is None
    d = inspect.signature(pbf.Context.plonk_prove_bn254_pi_dev).parameters
    assert list(d)[1:7] == ["n", "d_q", "d_copies", "d_abc", "d_pub", "npub"] and "stream" in d
    v = inspect.signature(pbf.Context.plonk_verify_bn254_pi).parameters
    assert list(v)[1:10] == ["q", "copies", "srs", "g2s", "pts", "fields", "pub", "chal", "u"]
    vd = inspect.signature(pbf.Context.plonk_verify_bn254_pi_dev).parameters
    assert list(vd)[1:6] == ["n", "d_q", "d_copies", "d_srs", "srs_m"] and "pub" in vd and "stream" in vd
    b = inspect.signature(pbf.Context.plonk_verify_bn254_batch_pi).parameters
    assert list(b)[1:10] == ["q", "copies", "srs", "g2s", "proofs", "pubs", "chals", "us", "rhos"]
    assert b["each"].default is False
    bd = inspect.signature(pbf.Context.plonk_verify_bn254_batch_pi_dev).parameters
    assert list(bd)[1:6] == ["n", "d_q", "d_copies", "d_srs", "srs_m"] and "pubs" in bd and "each" in bd


def test_batch_pub_is_proof_major_and_compact():
    import pbf
    import pytest

    pb, npub = pbf.Context._batch_pub([[1, 2, 1 << 200], [4, 5, 6]])
    assert npub == 3 and pb.shape == (24,)
    assert pb[0] == 1 and pb[4] == 2 and pb[8 + 3] == 1 << 8 and pb[12] == 4 and pb[20] == 6
    assert pbf.Context._batch_pub([[], []])[1] == 0
    with pytest.raises(ValueError):
        pbf.Context._batch_pub([[1, 2], [3]])


def test_pub_argument_of_one_statement():
    import pbf

    assert pbf.Context._pub_arg(None, None)[1:] == (None, 0)
    assert pbf.Context._pub_arg(None, 1)[1:] == (None, 1)  # the NULL-pub error case reaches the library
    a, p, npub = pbf.Context._pub_arg([7, 1 << 64], None)
    assert npub == 2 and a.tolist() == [7, 0, 0, 0, 0, 1, 0, 0] and p is not None
    assert pbf.Context._pub_arg([], None)[1:] == (None, 0)
