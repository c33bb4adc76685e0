"""The coset NTT / low-degree extension entry points are part of the C ABI: declared in
include/pbf.h, described in pbf.SIGNATURES and exported with C linkage (CPU only)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pbf.h")
COSET = ["pbf_ntt_u64_coset", "pbf_ntt_u64_coset_batch_dev", "pbf_ntt_fr256_coset", "pbf_ntt_fr256_coset_batch_dev"]


def test_coset_entry_points_declared_in_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(pbf_[a-z0-9_]+)\s*\(", src))
    for name in COSET:
        assert name in declared, name


def test_coset_entry_points_in_signatures():
    import pbf

    sigs = {n: (res, args) for n, res, args in pbf.SIGNATURES}
    for name in COSET:
        assert name in sigs, name
    # ctx, modulus, omega, shift, in, in_len, out, n, inverse (+ batch before it and a stream, _dev)
    assert len(sigs["pbf_ntt_u64_coset"][1]) == 9
    assert len(sigs["pbf_ntt_u64_coset_batch_dev"][1]) == 11
    # ctx, omega[4], shift[4], in, in_len, out, n, inverse
    assert len(sigs["pbf_ntt_fr256_coset"][1]) == 8
    assert len(sigs["pbf_ntt_fr256_coset_batch_dev"][1]) == 10
    for name in ("ntt_coset", "ntt_coset_batch_dev", "ntt_fr_coset", "ntt_fr_coset_batch_dev"):
        assert callable(getattr(pbf.Context, name)), name
    for name in ("coset_fft", "coset_fft_inv"):
        assert callable(getattr(pbf.CooleyTurkey, name)), name


def test_coset_entry_points_exported_with_c_linkage():
    import pbf

    out = subprocess.run(["nm", "-D", "--defined-only", pbf.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (pbf_[a-z0-9_]+)", out.stdout))
    for name in COSET:
        assert name in exported, name
