"""Python host binding of libpbf.so (the MI355X PLONK hot path, gfx950).

Mirrors the reference's FFT trait surface (src/fft.rs:6-21,109-132) and
Poly::eval (src/poly.rs:71-79) over the C-ABI declared in include/pbf.h.
This module is plumbing for tests and bench.py: every call goes through the HIP
library; there is no CPU fallback, and importing it without a built libpbf.so
raises immediately.
"""
from __future__ import annotations

import ctypes
import os
from typing import Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PBF_LIB: an alternative build of the library (A/B runs against another commit's libpbf.so)
LIB_PATH = os.environ.get("PBF_LIB") or os.path.join(os.path.dirname(_HERE), "libpbf.so")

GOLDILOCKS = 0xFFFFFFFF00000001

PBF_OK, PBF_EINVAL, PBF_ENOINV, PBF_EDEVICE, PBF_ECOMM, PBF_EUNSUPPORTED = range(6)
_NAMES = {1: "PBF_EINVAL", 2: "PBF_ENOINV", 3: "PBF_EDEVICE", 4: "PBF_ECOMM", 5: "PBF_EUNSUPPORTED"}


class PbfError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_NAMES.get(code, code)}: {msg}")
        self.code = code


_u64 = ctypes.c_uint64
_p64 = ctypes.POINTER(ctypes.c_uint64)
_sz = ctypes.c_size_t
_vp = ctypes.c_void_p
_p32 = ctypes.POINTER(ctypes.c_uint32)
_p8 = ctypes.POINTER(ctypes.c_uint8)
_pint = ctypes.POINTER(ctypes.c_int)

# (name, restype, argtypes) for every entry point in include/pbf.h
SIGNATURES = [
    ("pbf_ctx_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    ("pbf_ctx_destroy", None, [_vp]),
    ("pbf_last_error", ctypes.c_char_p, []),
    ("pbf_ctx_set_stream", ctypes.c_int, [_vp, _vp]),
    ("pbf_ctx_set_option", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_char_p]),
    ("pbf_device_sync", ctypes.c_int, [_vp]),
    ("pbf_ctx_release_caches", ctypes.c_int, [_vp]),
    ("pbf_ntt_u64", ctypes.c_int, [_vp, _u64, _u64, _p64, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_u64_batch_dev", ctypes.c_int, [_vp, _u64, _u64, _vp, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_mul_ntt_u64", ctypes.c_int, [_vp, _u64, _u64, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_poly_eval_u64", ctypes.c_int, [_vp, _u64, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_poly_add_u64", ctypes.c_int, [_vp, _u64, _p64, _sz, _p64, _sz, _p64, ctypes.POINTER(_sz)]),
    ("pbf_poly_sub_u64", ctypes.c_int, [_vp, _u64, _p64, _sz, _p64, _sz, _p64, ctypes.POINTER(_sz)]),
    ("pbf_poly_div_u64", ctypes.c_int, [_vp, _u64, _u64, ctypes.c_uint32, _p64, _sz, _p64, _sz, _p64,
                                        ctypes.POINTER(_sz), _p64, ctypes.POINTER(_sz)]),
    ("pbf_fill_random_u64_dev", ctypes.c_int, [_vp, _u64, _u64, _vp, _sz, _vp]),
    ("pbf_pointwise_mul_u64_dev", ctypes.c_int, [_vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    ("pbf_ntt_fr256_shard_local_dev", ctypes.c_int, [_vp, _p64, ctypes.c_uint32, _vp, _vp, _sz, _sz, ctypes.c_int,
                                                     _vp]),
    ("pbf_ntt_fr256_shard_combine_dev", ctypes.c_int, [_vp, _p64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _sz,
                                                       _sz, ctypes.c_int, _vp]),
    ("pbf_pointwise_mul_fr256_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp]),
    ("pbf_ntt_fr256", ctypes.c_int, [_vp, _p64, _p64, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_fr256_batch_dev", ctypes.c_int, [_vp, _p64, _vp, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_mul_ntt_fr256", ctypes.c_int, [_vp, _p64, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_mul_ntt_fr256_dev", ctypes.c_int, [_vp, _p64, _vp, _vp, _vp, _sz, _sz, _vp]),
    ("pbf_msm_g1_bn254", ctypes.c_int, [_vp, _p64, _p64, _sz, _p64]),
    ("pbf_msm_g1_bn254_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _p64, _vp]),
    ("pbf_g1_bn254_mul_base_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("pbf_msm_g1_bn254_fixed_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _p64, _vp]),
    ("pbf_srs_create_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64]),
    ("pbf_pairing_bn254", ctypes.c_int, [_vp, _p64, _p64, _sz, _p64]),
    ("pbf_pairing_bn254_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("pbf_pairing_check_bn254", ctypes.c_int, [_vp, _p64, _p64, _sz, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_g2_bn254_mul", ctypes.c_int, [_vp, _p64, _p64, _sz, _p64]),
    ("pbf_plonk_prove_bn254", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _p64, _p64, _p64, _p64, _sz, ctypes.c_int,
                                             _p64, _p64]),
    ("pbf_plonk_prove_bn254_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _p64, _p64, _p64, _vp, _sz, ctypes.c_int,
                                                 _p64, _p64, _vp]),
    ("pbf_plonk_verify_bn254", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _p64, _p64, _p64, _p64, _p64,
                                              ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_plonk_verify_bn254_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _p64, _p64, _p64, _p64, _p64,
                                                  ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp]),
    ("pbf_plonk_verify_bn254_batch", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _sz, _p64, _p64, _p64,
                                                    _p64, _p64, _p64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                    ctypes.POINTER(ctypes.c_int)]),
    ("pbf_plonk_verify_bn254_batch_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _sz, _p64, _p64, _p64,
                                                        _p64, _p64, _p64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                        ctypes.POINTER(ctypes.c_int), _vp]),
    ("pbf_plonk_prove_bn254_pi", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _p64, _sz, _p64, _p64, _p64, _p64, _sz,
                                                ctypes.c_int, _p64, _p64]),
    ("pbf_plonk_prove_bn254_pi_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _vp, _sz, _p64, _p64, _p64, _vp, _sz,
                                                    ctypes.c_int, _p64, _p64, _vp]),
    ("pbf_plonk_verify_bn254_pi", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _p64, _p64, _p64, _sz, _p64,
                                                 _p64, _p64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_plonk_verify_bn254_pi_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _p64, _p64, _p64, _sz, _p64,
                                                     _p64, _p64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp]),
    ("pbf_plonk_verify_bn254_batch_pi", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _sz, _p64, _p64, _p64,
                                                       _sz, _p64, _p64, _p64, _p64, ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("pbf_plonk_verify_bn254_batch_pi_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _sz, _p64, _p64, _p64,
                                                           _sz, _p64, _p64, _p64, _p64, ctypes.c_int,
                                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                           _vp]),
    ("pbf_keccak256_batch", ctypes.c_int, [_vp, _p8, _sz, _sz, _sz, _p8]),
    ("pbf_keccak256_batch_dev", ctypes.c_int, [_vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    ("pbf_plonk_circuit_digest_bn254", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _p64, ctypes.c_int, _sz,
                                                      _p8]),
    ("pbf_plonk_circuit_digest_bn254_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _p64, ctypes.c_int, _sz,
                                                          _p8, _vp]),
    ("pbf_plonk_challenges_bn254", ctypes.c_int, [_vp, _p8, _sz, _p64, _p64, _p64, _sz, _p64, _p64, _p64]),
    ("pbf_plonk_prove_bn254_fs", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _p64, _sz, _p8, _p64, _p64, _p64, _sz,
                                                ctypes.c_int, _p64, _p64, _p64]),
    ("pbf_plonk_prove_bn254_fs_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _vp, _sz, _p8, _p64, _p64, _vp, _sz,
                                                    ctypes.c_int, _p64, _p64, _p64, _vp]),
    ("pbf_plonk_verify_bn254_fs", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _p64, _p64, _p64, _sz, _p64,
                                                 ctypes.c_int, _pint]),
    ("pbf_plonk_verify_bn254_fs_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _p64, _p64, _p64, _sz, _p64,
                                                     ctypes.c_int, _pint, _vp]),
    ("pbf_plonk_verify_bn254_batch_fs", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _sz, _p64, _sz, _p64, _p64, _p64,
                                                       _sz, _p64, ctypes.c_int, _pint, _pint]),
    ("pbf_plonk_verify_bn254_batch_fs_dev", ctypes.c_int, [_vp, _sz, _vp, _vp, _vp, _sz, _p64, _sz, _p64, _p64, _p64,
                                                           _sz, _p64, ctypes.c_int, _pint, _pint, _vp]),
    ("pbf_plonk_prove_bn254_sharded_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _p64, _p64, _p64, _vp, _sz,
                                                         ctypes.c_int, _p64, _p64, _vp]),
    ("pbf_plonk_synth_circuit_bn254_dev", ctypes.c_int, [_vp, _sz, _u64, _vp, _vp, _vp, _vp]),
    ("pbf_srs_create_bn254_dev", ctypes.c_int, [_vp, _p64, _sz, _vp, _vp]),
    ("pbf_pbh_g1_mul", ctypes.c_int, [_vp, _p32, _p32, _sz, _p32]),
    ("pbf_pbh_g2_mul", ctypes.c_int, [_vp, _p32, _p32, _sz, _p32]),
    ("pbf_pbh_gt_pow", ctypes.c_int, [_vp, _p32, _p32, _sz, _p32]),
    ("pbf_pbh_pairing", ctypes.c_int, [_vp, _p32, _p32, _sz, _p32]),
    ("pbf_pbh_prove", ctypes.c_int, [_vp, _sz, _p64, _p64, _p64, _p64, _p64, _u64, _u64, _u64, _u64, _p64, _p64,
                                     ctypes.POINTER(ctypes.c_int)]),
    ("pbf_ntt_shard_local_dev", ctypes.c_int, [_vp, _u64, _u64, ctypes.c_uint32, _vp, _vp, _sz, _sz, ctypes.c_int,
                                               _vp]),
    ("pbf_ntt_shard_combine_dev", ctypes.c_int, [_vp, _u64, _u64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _sz,
                                                 _sz, ctypes.c_int, _vp]),
    ("pbf_ntt_u64_multi", ctypes.c_int, [_vp, ctypes.c_uint32, _u64, _u64, _p64, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_u64_multi_dev", ctypes.c_int, [_vp, ctypes.c_uint32, _u64, _u64, _vp, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_ntt_fr256_multi", ctypes.c_int, [_vp, ctypes.c_uint32, _p64, _p64, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_fr256_multi_dev", ctypes.c_int, [_vp, ctypes.c_uint32, _p64, _vp, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_mul_ntt_u64_multi", ctypes.c_int, [_vp, ctypes.c_uint32, _u64, _u64, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_mul_ntt_fr256_multi", ctypes.c_int, [_vp, ctypes.c_uint32, _p64, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_plonk_prove_bn254_multi", ctypes.c_int, [_vp, ctypes.c_uint32, _sz, _p64, _p64, _p64, _p64, _p64, _p64, _p64,
                                                   _sz, ctypes.c_int, _p64, _p64]),
    ("pbf_plonk_prove_bn254_multi_dev", ctypes.c_int, [_vp, ctypes.c_uint32, _sz, _vp, _vp, _vp, _p64, _p64, _p64, _vp,
                                                       _sz, ctypes.c_int, _p64, _p64, _vp]),
    ("pbf_multi_backend", ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_msm_g1_bn254_fixed_range_dev", ctypes.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _p64, _vp]),
    ("pbf_ntt_u64_coset", ctypes.c_int, [_vp, _u64, _u64, _u64, _p64, _sz, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_u64_coset_batch_dev", ctypes.c_int, [_vp, _u64, _u64, _u64, _vp, _sz, _vp, _sz, _sz, ctypes.c_int,
                                                   _vp]),
    ("pbf_ntt_fr256_coset", ctypes.c_int, [_vp, _p64, _p64, _p64, _sz, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_fr256_coset_batch_dev", ctypes.c_int, [_vp, _p64, _p64, _vp, _sz, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_poly_eval_fr256", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_kzg_commit_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _sz, _sz, _p64]),
    ("pbf_kzg_commit_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _p64, _vp]),
    ("pbf_kzg_open_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _sz, _sz, _p64, _p64, _p64, _p64]),
    ("pbf_kzg_open_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _p64, _p64, _p64, _p64, _vp]),
    ("pbf_kzg_verify_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _p64, _p64, _p64, _p64,
                                            ctypes.POINTER(ctypes.c_int)]),
    ("pbf_kzg_open_multi_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _sz, _sz, _p64, _sz, _p64, _p64, _p64,
                                                _p64]),
    ("pbf_kzg_open_multi_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _p64, _sz, _p64, _p64, _p64,
                                                    _p64, _vp]),
    ("pbf_kzg_open_multi_finish_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _sz, _sz, _p64, _sz, _p64, _p64,
                                                       _p64, _p64]),
    ("pbf_kzg_open_multi_finish_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _p64, _sz, _p64, _p64,
                                                           _p64, _p64, _vp]),
    ("pbf_kzg_verify_multi_bn254", ctypes.c_int, [_vp, _p64, _sz, _sz, _sz, _p64, _p64, _p64, _p64, _p64, _p64, _p64,
                                                  _p64, _p64, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_ntt_g1_bn254", ctypes.c_int, [_vp, _p64, _p64, _p64, _sz, ctypes.c_int]),
    ("pbf_ntt_g1_bn254_dev", ctypes.c_int, [_vp, _p64, _vp, _vp, _sz, ctypes.c_int, _vp]),
    ("pbf_ntt_g1_bn254_batch", ctypes.c_int, [_vp, _p64, _p64, _p64, _sz, _sz, ctypes.c_int]),
    ("pbf_ntt_g1_bn254_batch_dev", ctypes.c_int, [_vp, _p64, _vp, _vp, _sz, _sz, ctypes.c_int, _vp]),
    ("pbf_kzg_open_evals_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _p64, _sz, _sz, _p64, _p64, _p64, _p64]),
    ("pbf_kzg_open_evals_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _p64, _vp, _sz, _sz, _p64, _p64, _p64, _p64,
                                                    _vp]),
    ("pbf_g1_bn254_mul", ctypes.c_int, [_vp, _p64, _p64, _p64, _sz]),
    ("pbf_g1_bn254_mul_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp]),
    ("pbf_kzg_fk20_setup_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _p64]),
    ("pbf_kzg_fk20_setup_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _p64, _sz, _vp, _vp]),
    ("pbf_kzg_open_all_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _p64, _sz, _sz, _sz, _p64, _p64, _p64]),
    ("pbf_kzg_open_all_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _p64, _vp, _sz, _sz, _sz, _p64, _vp, _vp, _vp]),
    ("pbf_kzg_cells_setup_bn254", ctypes.c_int, [_vp, _p64, _sz, _p64, _sz, _sz, _p64]),
    ("pbf_kzg_cells_setup_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _p64, _sz, _sz, _vp, _vp]),
    ("pbf_kzg_open_cells_bn254", ctypes.c_int, [_vp, _p64, _sz, _sz, _p64, _p64, _sz, _sz, _sz, _p64, _p64, _p64]),
    ("pbf_kzg_open_cells_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _sz, _p64, _vp, _sz, _sz, _sz, _p64, _vp, _vp,
                                                    _vp]),
    ("pbf_kzg_open_cells_each_bn254", ctypes.c_int, [_vp, _p64, _sz, _sz, _p64, _p64, _sz, _sz, _sz, _p64, _p64]),
    ("pbf_kzg_open_cells_each_bn254_dev", ctypes.c_int, [_vp, _vp, _sz, _sz, _p64, _vp, _sz, _sz, _sz, _vp, _vp, _vp]),
    ("pbf_kzg_verify_cells_bn254",ctypes.c_int, [_vp, _p64, _p64, _sz, _p64, _sz, _sz, _sz, _p64, _p64, _p64, _p64,
                                                  _p64, ctypes.POINTER(ctypes.c_int)]),
    ("pbf_kzg_recover_cells_bn254", ctypes.c_int, [_vp, _p64, _sz, _sz, _sz, _sz, _p64, _p64, _sz, _p64, _sz, _p64,
                                                   ctypes.POINTER(ctypes.c_int)]),
    ("pbf_kzg_recover_cells_bn254_dev", ctypes.c_int, [_vp, _p64, _sz, _sz, _sz, _sz, _p64, _vp, _sz, _vp, _sz, _vp,
                                                       _vp, _vp]),
]

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libpbf.so (raises if it was not built: no fallback path exists)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch ships its own libamdhip64.so (SONAME
        # libamdhip64.so.7). Loading torch first makes libpbf.so's NEEDED
        # libamdhip64.so.7 bind to that copy instead of mapping /opt/rocm's as a
        # second runtime (two runtimes in one process cannot both own the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise ImportError(f"libpbf.so not built at {path}; run __graft_entry__.build()")
        lib = ctypes.CDLL(path)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc: int) -> None:
    if rc != PBF_OK:
        msg = load_library().pbf_last_error()
        raise PbfError(rc, msg.decode() if msg else "")


def _as_u64(x: Sequence[int] | np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
    return a


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_p64)


class Context:
    """pbf_ctx: one device, one stream, cached twiddle tables and scratch."""

    def __init__(self, device: int = 0, options: dict | None = None):
        lib = load_library()
        h = _vp()
        _check(lib.pbf_ctx_create(device, ctypes.byref(h)))
        self.h = h
        self.lib = lib
        self.device = device
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def close(self) -> None:
        if self.h:
            self.lib.pbf_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_caches(self) -> None:
        """pbf_ctx_release_caches: free the proving / verification keys, the fixed-base MSM
        window table, the pairing check's prepared lines and their validating copies."""
        _check(self.lib.pbf_ctx_release_caches(self.h))

    def set_stream(self, stream_ptr: int) -> None:
        _check(self.lib.pbf_ctx_set_stream(self.h, _vp(stream_ptr)))

    def set_option(self, name: str, value) -> None:
        """pbf_ctx_set_option (include/pbf.h): a context option such as "ntt.passes" = "12,12";
        None removes it. Cached plans are rebuilt under the new value."""
        _check(self.lib.pbf_ctx_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    def sync(self) -> None:
        _check(self.lib.pbf_device_sync(self.h))

    # fft.rs:66-78
    def ntt(self, modulus: int, omega: int, values, inverse: bool = False) -> np.ndarray:
        a = _as_u64(values)
        out = np.empty_like(a)
        _check(self.lib.pbf_ntt_u64(self.h, modulus, omega, _ptr(a), _ptr(out), a.size, int(inverse)))
        return out

    def ntt_batch_dev(self, modulus: int, omega: int, d_in: int, d_out: int, n: int, batch: int,
                      inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_u64_batch_dev(self.h, modulus, omega, _vp(d_in), _vp(d_out), n, batch,
                                              int(inverse), _vp(stream) if stream else None))

    # the same transforms on the coset shift * <omega> (include/pbf.h "coset NTT"): forward is the
    # low-degree extension of len(values) <= n coefficients to n evaluations
    def ntt_coset(self, modulus: int, omega: int, shift: int, values, n: int | None = None,
                  inverse: bool = False) -> np.ndarray:
        a = _as_u64(values)
        n = a.size if n is None else int(n)
        out = np.empty(n, dtype=np.uint64)
        _check(self.lib.pbf_ntt_u64_coset(self.h, modulus, omega, shift, _ptr(a), a.size, _ptr(out), n,
                                          int(inverse)))
        return out

    def ntt_coset_batch_dev(self, modulus: int, omega: int, shift: int, d_in: int, in_len: int, d_out: int, n: int,
                            batch: int, inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_u64_coset_batch_dev(self.h, modulus, omega, shift, _vp(d_in), in_len, _vp(d_out), n,
                                                    batch, int(inverse), _vp(stream) if stream else None))

    # fft.rs:109-132
    def mul_ntt(self, modulus: int, omega: int, a, b) -> np.ndarray:
        a = _as_u64(a)
        b = _as_u64(b)
        out = np.empty(a.size + b.size, dtype=np.uint64)
        _check(self.lib.pbf_mul_ntt_u64(self.h, modulus, omega, _ptr(a), a.size, _ptr(b), b.size, _ptr(out)))
        return out

    # poly.rs:71-79
    def poly_eval(self, modulus: int, coeffs, xs) -> np.ndarray:
        c = _as_u64(coeffs)
        x = _as_u64(xs)
        y = np.empty_like(x)
        _check(self.lib.pbf_poly_eval_u64(self.h, modulus, _ptr(c), c.size, _ptr(x), x.size, _ptr(y)))
        return y

    # poly.rs:165-203 AddAssign / SubAssign<&Poly> (normalised; sub keeps the :196 quirk)
    def poly_add(self, modulus: int, a, b) -> np.ndarray:
        return self._addsub(self.lib.pbf_poly_add_u64, modulus, a, b)

    def poly_sub(self, modulus: int, a, b) -> np.ndarray:
        return self._addsub(self.lib.pbf_poly_sub_u64, modulus, a, b)

    def _addsub(self, fn, modulus, a, b):
        x, y = _as_u64(a), _as_u64(b)
        out = np.empty(max(x.size, y.size), dtype=np.uint64)
        ln = _sz()
        _check(fn(self.h, modulus, _ptr(x), x.size, _ptr(y), y.size, _ptr(out), ctypes.byref(ln)))
        return out[: ln.value].copy()

    # poly.rs:230-247 Div for Poly -> (q, r); `root` of order 2^root_log bounds the NTT sizes
    def poly_div(self, modulus: int, num, den, root: int | None = None, root_log: int | None = None):
        if root is None:
            root, root_log = default_root(modulus)
        n, d = _as_u64(num), _as_u64(den)
        q = np.empty(max(n.size, 1), dtype=np.uint64)
        r = np.empty(max(n.size, 1), dtype=np.uint64)
        lq, lr = _sz(), _sz()
        _check(self.lib.pbf_poly_div_u64(self.h, modulus, root, root_log, _ptr(n), n.size, _ptr(d), d.size, _ptr(q),
                                         ctypes.byref(lq), _ptr(r), ctypes.byref(lr)))
        return q[: lq.value].copy(), r[: lr.value].copy()

    # multi-GPU stride-sharded NTT pieces (include/pbf.h)
    def shard_local_dev(self, modulus: int, omega: int, world: int, d_in: int, d_out: int, nl: int, batch: int,
                        inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_shard_local_dev(self.h, modulus, omega, world, _vp(d_in), _vp(d_out), nl, batch,
                                                int(inverse), _vp(stream) if stream else None))

    def shard_combine_dev(self, modulus: int, omega: int, world: int, rank: int, d_in: int, d_out: int, nl: int,
                          batch: int, inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_shard_combine_dev(self.h, modulus, omega, world, rank, _vp(d_in), _vp(d_out), nl,
                                                  batch, int(inverse), _vp(stream) if stream else None))

    def pointwise_mul_dev(self, modulus: int, d_a: int, d_b: int, d_c: int, count: int, stream: int = 0) -> None:
        _check(self.lib.pbf_pointwise_mul_u64_dev(self.h, modulus, _vp(d_a), _vp(d_b), _vp(d_c), count,
                                                  _vp(stream) if stream else None))

    def fr_shard_local_dev(self, omega: int, world: int, d_in: int, d_out: int, nl: int, batch: int,
                           inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_fr256_shard_local_dev(self.h, _ptr(ints_to_limbs([omega])), world, _vp(d_in),
                                                      _vp(d_out), nl, batch, int(inverse),
                                                      _vp(stream) if stream else None))

    def fr_shard_combine_dev(self, omega: int, world: int, rank: int, d_in: int, d_out: int, nl: int, batch: int,
                             inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_fr256_shard_combine_dev(self.h, _ptr(ints_to_limbs([omega])), world, rank,
                                                        _vp(d_in), _vp(d_out), nl, batch, int(inverse),
                                                        _vp(stream) if stream else None))

    def fr_pointwise_mul_dev(self, d_a: int, d_b: int, d_c: int, count: int, stream: int = 0) -> None:
        _check(self.lib.pbf_pointwise_mul_fr256_dev(self.h, _vp(d_a), _vp(d_b), _vp(d_c), count,
                                                    _vp(stream) if stream else None))

    # ---- BN254 Fr (elements as Python ints <-> 4 x u64 little-endian)
    def ntt_fr(self, omega: int, values, inverse: bool = False) -> list:
        a = ints_to_limbs(values)
        out = np.empty_like(a)
        w = ints_to_limbs([omega])
        _check(self.lib.pbf_ntt_fr256(self.h, _ptr(w), _ptr(a), _ptr(out), len(values), int(inverse)))
        return limbs_to_ints(out)

    def mul_ntt_fr(self, omega: int, a, b) -> list:
        la, lb = ints_to_limbs(a), ints_to_limbs(b)
        out = np.empty((len(a) + len(b)) * 4, dtype=np.uint64)
        w = ints_to_limbs([omega])
        _check(self.lib.pbf_mul_ntt_fr256(self.h, _ptr(w), _ptr(la), len(a), _ptr(lb), len(b), _ptr(out)))
        return limbs_to_ints(out)

    def ntt_fr_batch_dev(self, omega: int, d_in: int, d_out: int, n: int, batch: int, inverse: bool = False,
                         stream: int = 0) -> None:
        w = ints_to_limbs([omega])
        _check(self.lib.pbf_ntt_fr256_batch_dev(self.h, _ptr(w), _vp(d_in), _vp(d_out), n, batch, int(inverse),
                                                _vp(stream) if stream else None))

    def ntt_fr_coset(self, omega: int, shift: int, values, n: int | None = None, inverse: bool = False) -> list:
        a = ints_to_limbs(values)
        n = len(values) if n is None else int(n)
        out = np.empty(4 * n, dtype=np.uint64)
        _check(self.lib.pbf_ntt_fr256_coset(self.h, _ptr(ints_to_limbs([omega])), _ptr(ints_to_limbs([shift])),
                                            _ptr(a), len(values), _ptr(out), n, int(inverse)))
        return limbs_to_ints(out)

    def ntt_fr_coset_batch_dev(self, omega: int, shift: int, d_in: int, in_len: int, d_out: int, n: int, batch: int,
                               inverse: bool = False, stream: int = 0) -> None:
        _check(self.lib.pbf_ntt_fr256_coset_batch_dev(self.h, _ptr(ints_to_limbs([omega])),
                                                      _ptr(ints_to_limbs([shift])), _vp(d_in), in_len, _vp(d_out), n,
                                                      batch, int(inverse), _vp(stream) if stream else None))

    def mul_ntt_fr_dev(self, omega: int, d_a: int, d_b: int, d_out: int, n: int, batch: int, stream: int = 0):
        w = ints_to_limbs([omega])
        _check(self.lib.pbf_mul_ntt_fr256_dev(self.h, _ptr(w), _vp(d_a), _vp(d_b), _vp(d_out), n, batch,
                                              _vp(stream) if stream else None))

    # ---- BN254 G1 (points as (x, y) Python int pairs; identity = (0, 0))
    def msm_g1(self, points, scalars) -> tuple:
        pts = ints_to_limbs([c for pt in points for c in pt])
        sc = ints_to_limbs(scalars)
        out = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_msm_g1_bn254(self.h, _ptr(pts), _ptr(sc), len(scalars), _ptr(out)))
        x, y = limbs_to_ints(out)
        return (x, y)

    def msm_g1_dev(self, d_points: int, d_scalars: int, n: int, stream: int = 0) -> tuple:
        out = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_msm_g1_bn254_dev(self.h, _vp(d_points), _vp(d_scalars), n, _ptr(out),
                                             _vp(stream) if stream else None))
        x, y = limbs_to_ints(out)
        return (x, y)

    def msm_g1_fixed_dev(self, d_points: int, n_points: int, d_scalars: int, n: int, stream: int = 0) -> tuple:
        """sum_{i<n} s_i P_i against the fixed base set of n_points points (KZG commit)."""
        out = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_msm_g1_bn254_fixed_dev(self.h, _vp(d_points), n_points, _vp(d_scalars), n, _ptr(out),
                                                   _vp(stream) if stream else None))
        v = limbs_to_ints(out)
        return v[0], v[1]

    def msm_g1_fixed_range_dev(self, d_points: int, n_points: int, first: int, d_scalars: int, n: int,
                               stream: int = 0) -> tuple:
        """sum_{i<n} s_i P_(first+i) against the fixed base set (one rank's point range)."""
        out = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_msm_g1_bn254_fixed_range_dev(self.h, _vp(d_points), n_points, first, _vp(d_scalars), n,
                                                         _ptr(out), _vp(stream) if stream else None))
        v = limbs_to_ints(out)
        return v[0], v[1]

    def g1_mul_base_dev(self, d_scalars: int, d_out: int, n: int, stream: int = 0) -> None:
        _check(self.lib.pbf_g1_bn254_mul_base_dev(self.h, _vp(d_scalars), _vp(d_out), n,
                                                  _vp(stream) if stream else None))

    def srs_create(self, s: int, n: int) -> list:
        out = np.zeros((n + 1) * 8, dtype=np.uint64)
        _check(self.lib.pbf_srs_create_bn254(self.h, _ptr(ints_to_limbs([s])), n, _ptr(out)))
        v = limbs_to_ints(out)
        return [(v[2 * i], v[2 * i + 1]) for i in range(n + 1)]

    # ---- generalised PLONK over BN254 (config 5; prover.hip)
    def plonk_prove_bn254(self, q, copies, abc, chal, rnd, srs, k1k2=(2, 3), mode=0):
        """q: 5 columns (q_l, q_r, q_o, q_m, q_c) of n ints; copies: 3 columns of (kind, 1-based
        idx); abc: 3 columns; chal: (alpha, beta, gamma, z, v); rnd: b1..b9; srs: affine points.
        Returns (9 points, 7 field ints) as Proof (plonk.rs:61-95)."""
        n = len(abc[0])
        qa, ca, aa, sa = _circuit_limbs(q, copies, srs, abc)
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254(self.h, n, _ptr(qa), _ptr(ca), _ptr(aa), _ptr(ints_to_limbs(chal)),
                                              _ptr(ints_to_limbs(rnd)), _ptr(ints_to_limbs(k1k2)), _ptr(sa), len(srs),
                                              mode, _ptr(pts), _ptr(fs)))
        pv = limbs_to_ints(pts)
        return [None if pv[2 * i] == 0 and pv[2 * i + 1] == 0 else (pv[2 * i], pv[2 * i + 1]) for i in range(9)], \
            limbs_to_ints(fs)

    def plonk_verify_bn254(self, q, copies, srs, g2s, pts, fields, chal, u, k1k2=(2, 3), mode=0) -> bool:
        return self.plonk_verify_bn254_pi(q, copies, srs, g2s, pts, fields, None, chal, u, k1k2, mode)

    def plonk_synth_circuit_dev(self, n, seed, d_q, d_copies, d_abc, stream: int = 0) -> None:
        _check(self.lib.pbf_plonk_synth_circuit_bn254_dev(self.h, n, seed, d_q, d_copies, d_abc, stream))

    def srs_create_dev(self, s: int, n: int, d_out: int, stream: int = 0) -> None:
        _check(self.lib.pbf_srs_create_bn254_dev(self.h, _ptr(ints_to_limbs([s])), n, d_out, stream))

    def plonk_prove_bn254_dev(self, n, d_q, d_copies, d_abc, chal, rnd, d_srs, srs_m, k1k2=(2, 3), mode=0,
                              stream: int = 0):
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_dev(self.h, n, d_q, d_copies, d_abc, _ptr(ints_to_limbs(chal)),
                                                  _ptr(ints_to_limbs(rnd)), _ptr(ints_to_limbs(k1k2)), d_srs, srs_m,
                                                  mode, _ptr(pts), _ptr(fs), stream))
        return pts, fs

    def plonk_verify_bn254_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, pts, fields, chal, u, k1k2=(2, 3),
                               mode=0, stream: int = 0) -> bool:
        """Plonk::verify (plonk.rs:468-650) with the circuit and SRS on the device; pts / fields
        as plonk_prove_bn254_dev returns them (limb arrays) or as ints / points."""
        return self.plonk_verify_bn254_pi_dev(n, d_q, d_copies, d_srs, srs_m, g2s, pts, fields, None, chal, u, k1k2,
                                              mode, stream)

    @staticmethod
    def _batch_arrays(proofs, chals, us, rhos):
        """Proof-major limb arrays of a batch: proofs a list of (pts, fields) as the provers return
        them (points / ints, or limb arrays); chals a list of 5-tuples; us, rhos lists of ints."""
        count = len(proofs)
        if not (len(chals) == len(us) == len(rhos) == count):
            raise ValueError("proofs, chals, us and rhos must have one entry per proof")
        pa = np.zeros(72 * count, dtype=np.uint64)
        fa = np.zeros(28 * count, dtype=np.uint64)
        for i, (pts, fields) in enumerate(proofs):
            pa[72 * i:72 * i + 72], fa[28 * i:28 * i + 28] = _proof_limbs(pts, fields)
        ca = ints_to_limbs([x for ch in chals for x in ch]) if count else np.zeros(0, dtype=np.uint64)
        ua = ints_to_limbs(list(us)) if count else np.zeros(0, dtype=np.uint64)
        ra = ints_to_limbs(list(rhos)) if count else np.zeros(0, dtype=np.uint64)
        return count, pa, fa, ca, ua, ra

    def plonk_verify_bn254_batch(self, q, copies, srs, g2s, proofs, chals, us, rhos, k1k2=(2, 3), mode=0,
                                 each=False):
        """pbf_plonk_verify_bn254_batch: many proofs of one circuit, one pairing check. rhos are the
        batching weights: nonzero, < r, chosen unpredictably after seeing the proofs (soundness
        rests on that; include/pbf.h). Returns ok, or (ok, [ok_i]) with each=True."""
        return self.plonk_verify_bn254_batch_pi(q, copies, srs, g2s, proofs, [()] * len(proofs), chals, us, rhos, k1k2,
                                                mode, each)

    def plonk_verify_bn254_batch_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, proofs, chals, us, rhos,
                                     k1k2=(2, 3), mode=0, each=False, stream: int = 0):
        """The same with the circuit and SRS on the device (shaped like plonk_verify_bn254_dev)."""
        return self.plonk_verify_bn254_batch_pi_dev(n, d_q, d_copies, d_srs, srs_m, g2s, proofs, [()] * len(proofs),
                                                    chals, us, rhos, k1k2, mode, each, stream)

    # ---- public inputs (include/pbf.h "Public inputs"): pub_i on gate row i < npub, one circuit for
    # many statements. pub: ints (or None with npub = 0); npub defaults to len(pub).
    @staticmethod
    def _pub_arg(pub, npub):
        """(limb array kept alive by the caller, its pointer or None, npub) of one statement."""
        if pub is None:
            return None, None, (0 if npub is None else npub)
        a = ints_to_limbs(list(pub))
        return a, (_ptr(a) if len(a) else None), (len(pub) if npub is None else npub)

    @staticmethod
    def _batch_pub(pubs):
        """count x npub x 4 limbs, proof-major and compact, of a batch's public inputs (one list per
        proof, all of one length); returns (array, npub)."""
        npub = len(pubs[0]) if pubs else 0
        if any(len(p) != npub for p in pubs):
            raise ValueError("every proof of a batch has the same number of public inputs")
        return ints_to_limbs([x for p in pubs for x in p]), npub

    def plonk_prove_bn254_pi(self, q, copies, abc, pub, chal, rnd, srs, k1k2=(2, 3), mode=0, npub=None):
        """plonk_prove_bn254 with public inputs: row i < npub satisfies ... + q_c - pub_i = 0."""
        n = len(abc[0])
        qa, ca, aa, sa = _circuit_limbs(q, copies, srs, abc)
        _keep, pp, npub = self._pub_arg(pub, npub)
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_pi(self.h, n, _ptr(qa), _ptr(ca), _ptr(aa), pp, npub,
                                                 _ptr(ints_to_limbs(chal)), _ptr(ints_to_limbs(rnd)),
                                                 _ptr(ints_to_limbs(k1k2)), _ptr(sa), len(srs), mode, _ptr(pts),
                                                 _ptr(fs)))
        pv = limbs_to_ints(pts)
        return [None if pv[2 * i] == 0 and pv[2 * i + 1] == 0 else (pv[2 * i], pv[2 * i + 1]) for i in range(9)], \
            limbs_to_ints(fs)

    def plonk_prove_bn254_pi_dev(self, n, d_q, d_copies, d_abc, d_pub, npub, chal, rnd, d_srs, srs_m, k1k2=(2, 3),
                                 mode=0, stream: int = 0):
        """The same on device inputs; d_pub: npub x 4 u64 on the device (0 / None with npub = 0)."""
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_pi_dev(self.h, n, d_q, d_copies, d_abc, d_pub or None, npub,
                                                     _ptr(ints_to_limbs(chal)), _ptr(ints_to_limbs(rnd)),
                                                     _ptr(ints_to_limbs(k1k2)), d_srs, srs_m, mode, _ptr(pts), _ptr(fs),
                                                     stream))
        return pts, fs

    def plonk_verify_bn254_pi(self, q, copies, srs, g2s, pts, fields, pub, chal, u, k1k2=(2, 3), mode=0,
                              npub=None) -> bool:
        n = len(q[0])
        qa, ca, sa = _circuit_limbs(q, copies, srs)
        pa, fa = _proof_limbs(pts, fields)
        _keep, pp, npub = self._pub_arg(pub, npub)
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_plonk_verify_bn254_pi(self.h, n, _ptr(qa), _ptr(ca), _ptr(sa), len(srs),
                                                  _ptr(_g2_limbs(g2s)), _ptr(pa), _ptr(fa), pp, npub,
                                                  _ptr(ints_to_limbs(chal)),
                                                  _ptr(ints_to_limbs([u])), _ptr(ints_to_limbs(k1k2)), mode,
                                                  ctypes.byref(ok)))
        return ok.value == 1

    def plonk_verify_bn254_pi_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, pts, fields, pub, chal, u, k1k2=(2, 3),
                                  mode=0, stream: int = 0, npub=None) -> bool:
        """The circuit and SRS on the device; the proof and pub on the host."""
        pa, fa = _proof_limbs(pts, fields)
        _keep, pp, npub = self._pub_arg(pub, npub)
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_plonk_verify_bn254_pi_dev(self.h, n, d_q, d_copies, d_srs, srs_m, _ptr(_g2_limbs(g2s)),
                                                      _ptr(pa), _ptr(fa), pp, npub,
                                                      _ptr(ints_to_limbs(chal)), _ptr(ints_to_limbs([u])),
                                                      _ptr(ints_to_limbs(k1k2)), mode, ctypes.byref(ok), stream))
        return ok.value == 1

    def plonk_verify_bn254_batch_pi(self, q, copies, srs, g2s, proofs, pubs, chals, us, rhos, k1k2=(2, 3), mode=0,
                                    each=False):
        """plonk_verify_bn254_batch over proofs of one circuit with a statement each: pubs[i] the
        public inputs of proofs[i]."""
        n = len(q[0])
        qa, ca, sa = _circuit_limbs(q, copies, srs)
        count, pa, fa, cha, ua, ra = self._batch_arrays(proofs, chals, us, rhos)
        if len(pubs) != count:
            raise ValueError("one list of public inputs per proof")
        pb, npub = self._batch_pub(pubs)
        ok = ctypes.c_int(-1)
        oe = (ctypes.c_int * max(count, 1))() if each else None
        _check(self.lib.pbf_plonk_verify_bn254_batch_pi(self.h, n, _ptr(qa), _ptr(ca), _ptr(sa), len(srs),
                                                        _ptr(_g2_limbs(g2s)), count, _ptr(pa), _ptr(fa),
                                                        _ptr(pb) if npub else None, npub, _ptr(cha), _ptr(ua),
                                                        _ptr(ra), _ptr(ints_to_limbs(k1k2)), mode, ctypes.byref(ok),
                                                        oe))
        return (ok.value == 1, [bool(v) for v in oe[:count]]) if each else ok.value == 1

    def plonk_verify_bn254_batch_pi_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, proofs, pubs, chals, us, rhos,
                                        k1k2=(2, 3), mode=0, each=False, stream: int = 0):
        """The same with the circuit and SRS on the device."""
        count, pa, fa, cha, ua, ra = self._batch_arrays(proofs, chals, us, rhos)
        if len(pubs) != count:
            raise ValueError("one list of public inputs per proof")
        pb, npub = self._batch_pub(pubs)
        ok = ctypes.c_int(-1)
        oe = (ctypes.c_int * max(count, 1))() if each else None
        _check(self.lib.pbf_plonk_verify_bn254_batch_pi_dev(self.h, n, d_q, d_copies, d_srs, srs_m,
                                                            _ptr(_g2_limbs(g2s)), count, _ptr(pa), _ptr(fa),
                                                            _ptr(pb) if npub else None, npub, _ptr(cha), _ptr(ua),
                                                            _ptr(ra), _ptr(ints_to_limbs(k1k2)), mode,
                                                            ctypes.byref(ok), oe, stream))
        return (ok.value == 1, [bool(v) for v in oe[:count]]) if each else ok.value == 1

    # ---- Fiat-Shamir (include/pbf.h "Fiat-Shamir"; transcript.hip): digests are 32 bytes
    @staticmethod
    def _digest_arg(digest):
        a = np.frombuffer(bytes(digest), dtype=np.uint8).copy()
        if a.size != 32:
            raise ValueError("a circuit digest is 32 bytes")
        return a

    def keccak256_batch(self, msgs, pitch: int | None = None) -> list:
        """Keccak-256 of byte strings of one length, laid out `pitch` bytes apart (default: compact)."""
        count, ln = len(msgs), (len(msgs[0]) if msgs else 0)
        if any(len(m) != ln for m in msgs):
            raise ValueError("every message of a batch has the same length")
        pitch = ln if pitch is None else pitch
        buf = np.zeros(max(count * max(pitch, ln), 1), dtype=np.uint8)
        for i, m in enumerate(msgs):
            buf[i * pitch:i * pitch + ln] = np.frombuffer(bytes(m), dtype=np.uint8)
        out = np.zeros(max(count, 1) * 32, dtype=np.uint8)
        _check(self.lib.pbf_keccak256_batch(self.h, buf.ctypes.data_as(_p8), count, ln, pitch, out.ctypes.data_as(_p8)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(count)]

    def keccak256_batch_dev(self, d_msgs: int, count: int, length: int, pitch: int, d_out: int, stream: int = 0):
        _check(self.lib.pbf_keccak256_batch_dev(self.h, d_msgs, count, length, pitch, d_out, stream))

    def plonk_circuit_digest_bn254(self, q, copies, srs, g2s, npub: int, k1k2=(2, 3), mode=0) -> bytes:
        """h0 of the transcript: the circuit's verification key, k1 k2, mode, n, npub and [s]G2."""
        n = len(q[0])
        qa, ca, sa = _circuit_limbs(q, copies, srs)
        out = np.zeros(32, dtype=np.uint8)
        _check(self.lib.pbf_plonk_circuit_digest_bn254(self.h, n, _ptr(qa), _ptr(ca), _ptr(sa), len(srs),
                                                       _ptr(_g2_limbs(g2s)), _ptr(ints_to_limbs(k1k2)), mode, npub,
                                                       out.ctypes.data_as(_p8)))
        return out.tobytes()

    def plonk_circuit_digest_bn254_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, npub: int, k1k2=(2, 3), mode=0,
                                       stream: int = 0) -> bytes:
        out = np.zeros(32, dtype=np.uint8)
        _check(self.lib.pbf_plonk_circuit_digest_bn254_dev(self.h, n, d_q, d_copies, d_srs, srs_m, _ptr(_g2_limbs(g2s)),
                                                           _ptr(ints_to_limbs(k1k2)), mode, npub,
                                                           out.ctypes.data_as(_p8), stream))
        return out.tobytes()

    def plonk_challenges_bn254(self, digest, proofs, pubs, rho: bool = True):
        """The transcript's challenges of a batch: ([alpha beta gamma z v] per proof, [u], [rho] or
        None). proofs: (pts, fields) pairs; pubs: one list of public inputs per proof."""
        count, pa, fa, pb, npub = self._batch_fs_arrays(proofs, pubs)
        d = self._digest_arg(digest)
        ca = np.zeros(20 * max(count, 1), dtype=np.uint64)
        ua = np.zeros(4 * max(count, 1), dtype=np.uint64)
        ra = np.zeros(4 * max(count, 1), dtype=np.uint64) if rho else None
        _check(self.lib.pbf_plonk_challenges_bn254(self.h, d.ctypes.data_as(_p8), count, _ptr(pa), _ptr(fa),
                                                   _ptr(pb) if npub else None, npub, _ptr(ca), _ptr(ua),
                                                   _ptr(ra) if rho else None))
        cv = limbs_to_ints(ca)
        return [cv[5 * i:5 * i + 5] for i in range(count)], limbs_to_ints(ua)[:count], \
            (limbs_to_ints(ra)[:count] if rho else None)

    def plonk_prove_bn254_fs(self, q, copies, abc, pub, digest, rnd, srs, k1k2=(2, 3), mode=0, npub=None):
        """plonk_prove_bn254_pi with the challenges derived from the transcript under `digest`
        (plonk_circuit_digest_bn254). Returns (9 points, 7 fields, [alpha beta gamma z v u])."""
        n = len(abc[0])
        qa, ca, aa, sa = _circuit_limbs(q, copies, srs, abc)
        _keep, pp, npub = self._pub_arg(pub, npub)
        d = self._digest_arg(digest)
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        ch = np.zeros(24, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_fs(self.h, n, _ptr(qa), _ptr(ca), _ptr(aa), pp, npub,
                                                 d.ctypes.data_as(_p8), _ptr(ints_to_limbs(rnd)),
                                                 _ptr(ints_to_limbs(k1k2)), _ptr(sa), len(srs), mode, _ptr(pts), _ptr(fs),
                                                 _ptr(ch)))
        pv = limbs_to_ints(pts)
        return [None if pv[2 * i] == 0 and pv[2 * i + 1] == 0 else (pv[2 * i], pv[2 * i + 1]) for i in range(9)], \
            limbs_to_ints(fs), limbs_to_ints(ch)

    def plonk_prove_bn254_fs_dev(self, n, d_q, d_copies, d_abc, d_pub, npub, digest, rnd, d_srs, srs_m, k1k2=(2, 3),
                                 mode=0, stream: int = 0):
        """The same on device inputs; returns (pts limbs, field limbs, challenge limbs 6 x 4)."""
        d = self._digest_arg(digest)
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        ch = np.zeros(24, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_fs_dev(self.h, n, d_q, d_copies, d_abc, d_pub or None, npub,
                                                     d.ctypes.data_as(_p8), _ptr(ints_to_limbs(rnd)),
                                                     _ptr(ints_to_limbs(k1k2)), d_srs, srs_m, mode, _ptr(pts), _ptr(fs),
                                                     _ptr(ch), stream))
        return pts, fs, ch

    def plonk_verify_bn254_fs(self, q, copies, srs, g2s, pts, fields, pub, k1k2=(2, 3), mode=0, npub=None) -> bool:
        n = len(q[0])
        qa, ca, sa = _circuit_limbs(q, copies, srs)
        pa, fa = _proof_limbs(pts, fields)
        _keep, pp, npub = self._pub_arg(pub, npub)
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_plonk_verify_bn254_fs(self.h, n, _ptr(qa), _ptr(ca), _ptr(sa), len(srs),
                                                  _ptr(_g2_limbs(g2s)), _ptr(pa), _ptr(fa), pp, npub,
                                                  _ptr(ints_to_limbs(k1k2)), mode, ctypes.byref(ok)))
        return ok.value == 1

    def plonk_verify_bn254_fs_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, pts, fields, pub, k1k2=(2, 3), mode=0,
                                  stream: int = 0, npub=None) -> bool:
        pa, fa = _proof_limbs(pts, fields)
        _keep, pp, npub = self._pub_arg(pub, npub)
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_plonk_verify_bn254_fs_dev(self.h, n, d_q, d_copies, d_srs, srs_m, _ptr(_g2_limbs(g2s)),
                                                      _ptr(pa), _ptr(fa), pp, npub, _ptr(ints_to_limbs(k1k2)), mode,
                                                      ctypes.byref(ok), stream))
        return ok.value == 1

    def _batch_fs_arrays(self, proofs, pubs):
        count = len(proofs)
        pa = np.zeros(72 * max(count, 1), dtype=np.uint64)
        fa = np.zeros(28 * max(count, 1), dtype=np.uint64)
        for i, (pts, fields) in enumerate(proofs):
            pa[72 * i:72 * i + 72], fa[28 * i:28 * i + 28] = _proof_limbs(pts, fields)
        if len(pubs) != count:
            raise ValueError("one list of public inputs per proof")
        pb, npub = self._batch_pub(pubs)
        return count, pa, fa, pb, npub

    def plonk_verify_bn254_batch_fs(self, q, copies, srs, g2s, proofs, pubs, k1k2=(2, 3), mode=0, each=False):
        """plonk_verify_bn254_batch_pi with chal, u and rho derived on the device from the transcript."""
        n = len(q[0])
        qa, ca, sa = _circuit_limbs(q, copies, srs)
        count, pa, fa, pb, npub = self._batch_fs_arrays(proofs, pubs)
        ok = ctypes.c_int(-1)
        oe = (ctypes.c_int * max(count, 1))() if each else None
        _check(self.lib.pbf_plonk_verify_bn254_batch_fs(self.h, n, _ptr(qa), _ptr(ca), _ptr(sa), len(srs),
                                                        _ptr(_g2_limbs(g2s)), count, _ptr(pa), _ptr(fa),
                                                        _ptr(pb) if npub else None, npub, _ptr(ints_to_limbs(k1k2)), mode,
                                                        ctypes.byref(ok), oe))
        return (ok.value == 1, [bool(v) for v in oe[:count]]) if each else ok.value == 1

    def plonk_verify_bn254_batch_fs_dev(self, n, d_q, d_copies, d_srs, srs_m, g2s, proofs, pubs, k1k2=(2, 3), mode=0,
                                        each=False, stream: int = 0):
        count, pa, fa, pb, npub = self._batch_fs_arrays(proofs, pubs)
        ok = ctypes.c_int(-1)
        oe = (ctypes.c_int * max(count, 1))() if each else None
        _check(self.lib.pbf_plonk_verify_bn254_batch_fs_dev(self.h, n, d_q, d_copies, d_srs, srs_m,
                                                            _ptr(_g2_limbs(g2s)), count, _ptr(pa), _ptr(fa),
                                                            _ptr(pb) if npub else None, npub, _ptr(ints_to_limbs(k1k2)),
                                                            mode, ctypes.byref(ok), oe, stream))
        return (ok.value == 1, [bool(v) for v in oe[:count]]) if each else ok.value == 1

    # ---- KZG commitments over BN254 (include/pbf.h "KZG commitments"; kzg.hip)
    def poly_eval_fr(self, coeffs, xs) -> list:
        """Poly::eval (poly.rs:71-79) over Fr: [p(x) for x in xs], ints in and out."""
        c, x = ints_to_limbs(coeffs), ints_to_limbs(xs)
        y = np.zeros(4 * len(xs), dtype=np.uint64)
        _check(self.lib.pbf_poly_eval_fr256(self.h, _ptr(c), len(coeffs), _ptr(x), len(xs), _ptr(y)))
        return limbs_to_ints(y)

    @staticmethod
    def _poly_limbs(polys, pitch):
        """A list of equal-length coefficient lists as one limb array, polynomial b at b * pitch."""
        batch = len(polys)
        ln = len(polys[0]) if batch else 0
        if any(len(p) != ln for p in polys):
            raise ValueError("the polynomials of one call have one length")
        pitch = ln if pitch is None else int(pitch)
        a = np.zeros(4 * max(pitch, ln) * max(batch, 1), dtype=np.uint64)
        for b, p in enumerate(polys):
            a[4 * b * pitch:4 * (b * pitch + ln)] = ints_to_limbs(p)
        return a, ln, pitch, batch

    @staticmethod
    def _points(out) -> list:
        v = limbs_to_ints(out)
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    def kzg_commit(self, srs, polys, pitch: int | None = None) -> list:
        """SRS::eval_at_s (plonk.rs:51-58) of each polynomial (lists of ints of one length);
        points as (x, y), the identity (0, 0)."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        out = np.zeros(8 * max(batch, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_commit_bn254(self.h, _ptr(_g1_limbs(srs)), len(srs), _ptr(a), ln, pitch, batch,
                                             _ptr(out)))
        return self._points(out)[:batch]

    def kzg_commit_dev(self, d_srs: int, srs_m: int, d_polys: int, length: int, pitch: int, batch: int,
                       stream: int = 0) -> list:
        out = np.zeros(8 * max(batch, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_commit_bn254_dev(self.h, _vp(d_srs), srs_m, _vp(d_polys), length, pitch, batch,
                                                 _ptr(out), _vp(stream) if stream else None))
        return self._points(out)[:batch]

    def kzg_open(self, srs, polys, z: int, weights, pitch: int | None = None):
        """The batched opening at z: ([p_b(z)], W) with W the commitment of
        (sum_b weights_b (p_b(x) - p_b(z))) / (x - z) (plonk.rs:429-446)."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        ys = np.zeros(4 * max(batch, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_bn254(self.h, _ptr(_g1_limbs(srs)), len(srs), _ptr(a), ln, pitch, batch,
                                           _ptr(ints_to_limbs([z])), _ptr(ints_to_limbs(list(weights))), _ptr(ys),
                                           _ptr(w)))
        return limbs_to_ints(ys)[:batch], self._points(w)[0]

    def kzg_open_dev(self, d_srs: int, srs_m: int, d_polys: int, length: int, pitch: int, batch: int, z: int,
                     weights, stream: int = 0):
        ys = np.zeros(4 * max(batch, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_bn254_dev(self.h, _vp(d_srs), srs_m, _vp(d_polys), length, pitch, batch,
                                               _ptr(ints_to_limbs([z])), _ptr(ints_to_limbs(list(weights))),
                                               _ptr(ys), _ptr(w), _vp(stream) if stream else None))
        return limbs_to_ints(ys)[:batch], self._points(w)[0]

    def kzg_verify(self, g2s, entries, rhos) -> bool:
        """pbf_kzg_verify_bn254: entries a list of (C, z, y, W); rhos the batching weights: nonzero,
        < r, chosen unpredictably after seeing the openings (soundness rests on that;
        include/pbf.h). One pairing check whatever the count."""
        if len(entries) != len(rhos):
            raise ValueError("one rho per entry")
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_kzg_verify_bn254(self.h, _ptr(_g2_limbs(g2s)), len(entries),
                                             _ptr(_g1_limbs([e[0] for e in entries])),
                                             _ptr(ints_to_limbs([e[1] for e in entries])),
                                             _ptr(ints_to_limbs([e[2] for e in entries])),
                                             _ptr(_g1_limbs([e[3] for e in entries])),
                                             _ptr(ints_to_limbs(list(rhos))), ctypes.byref(ok)))
        return ok.value == 1

    # ---- multi-point openings (include/pbf.h "Multi-point KZG openings"; kzg_multi.hip)
    @staticmethod
    def _sets(sets) -> np.ndarray:
        return np.array([int(m) for m in sets], dtype=np.uint64)

    def _multi_ys(self, ys, batch, npts) -> list:
        v = limbs_to_ints(ys)
        return [v[b * npts:(b + 1) * npts] for b in range(batch)]

    def kzg_open_multi(self, srs, polys, pts, sets, gamma: int, pitch: int | None = None):
        """pbf_kzg_open_multi_bn254, phase 1 of the multi-point opening: polynomial b is opened on
        the points t_j of pts whose bit j is set in sets[b]. (ys, W): ys[b][j] = p_b(t_j) inside
        the set and 0 outside. gamma is the caller's challenge, derived after the commitments and
        the evaluations (include/pbf.h)."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        npts = len(pts)
        ys = np.zeros(4 * max(batch * npts, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_multi_bn254(self.h, _ptr(_g1_limbs(srs) if len(srs) else np.zeros(8, np.uint64)),
                                                 len(srs), _ptr(a), ln, pitch, batch,
                                                 _ptr(ints_to_limbs(list(pts))), npts, _ptr(self._sets(sets)),
                                                 _ptr(ints_to_limbs([gamma])), _ptr(ys), _ptr(w)))
        return self._multi_ys(ys, batch, npts), self._points(w)[0]

    def kzg_open_multi_dev(self, d_srs: int, srs_m: int, d_polys: int, length: int, pitch: int, batch: int, pts, sets,
                           gamma: int, stream: int = 0):
        npts = len(pts)
        ys = np.zeros(4 * max(batch * npts, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_multi_bn254_dev(self.h, _vp(d_srs), srs_m, _vp(d_polys), length, pitch, batch,
                                                     _ptr(ints_to_limbs(list(pts))), npts, _ptr(self._sets(sets)),
                                                     _ptr(ints_to_limbs([gamma])), _ptr(ys), _ptr(w),
                                                     _vp(stream) if stream else None))
        return self._multi_ys(ys, batch, npts), self._points(w)[0]

    def kzg_open_multi_finish(self, srs, polys, pts, sets, gamma: int, z: int, pitch: int | None = None):
        """pbf_kzg_open_multi_finish_bn254, phase 2: W' for the challenge z, which the caller derives
        after W. Stateless: the arguments of kzg_open_multi again, and z."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        w2 = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_multi_finish_bn254(
            self.h, _ptr(_g1_limbs(srs) if len(srs) else np.zeros(8, np.uint64)), len(srs), _ptr(a), ln, pitch, batch,
            _ptr(ints_to_limbs(list(pts))), len(pts), _ptr(self._sets(sets)), _ptr(ints_to_limbs([gamma])),
            _ptr(ints_to_limbs([z])), _ptr(w2)))
        return self._points(w2)[0]

    def kzg_open_multi_finish_dev(self, d_srs: int, srs_m: int, d_polys: int, length: int, pitch: int, batch: int, pts,
                                  sets, gamma: int, z: int, stream: int = 0):
        w2 = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_multi_finish_bn254_dev(
            self.h, _vp(d_srs), srs_m, _vp(d_polys), length, pitch, batch, _ptr(ints_to_limbs(list(pts))), len(pts),
            _ptr(self._sets(sets)), _ptr(ints_to_limbs([gamma])), _ptr(ints_to_limbs([z])), _ptr(w2),
            _vp(stream) if stream else None))
        return self._points(w2)[0]

    def kzg_verify_multi(self, g2s, sets, openings, rhos) -> bool:
        """pbf_kzg_verify_multi_bn254: openings of one shape, each (commits, pts, ys, gamma, z, W, W')
        with ys[b][j] as kzg_open_multi returns it (entries outside a set are not read); rhos the
        batching weights: nonzero, < r, chosen unpredictably after seeing the openings (soundness
        rests on that; include/pbf.h). One pairing check whatever the count."""
        if len(openings) != len(rhos):
            raise ValueError("one rho per opening")
        batch = len(sets)
        npts = len(openings[0][1]) if openings else 0
        if any(len(o[0]) != batch or len(o[1]) != npts or len(o[2]) != batch or any(len(r) != npts for r in o[2])
               for o in openings):
            raise ValueError("the openings of one call have one shape")
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_kzg_verify_multi_bn254(
            self.h, _ptr(_g2_limbs(g2s)), len(openings), batch, npts, _ptr(self._sets(sets)),
            _ptr(_g1_limbs([c for o in openings for c in o[0]])),
            _ptr(ints_to_limbs([t for o in openings for t in o[1]])),
            _ptr(ints_to_limbs([v for o in openings for r in o[2] for v in r])),
            _ptr(ints_to_limbs([o[3] for o in openings])), _ptr(ints_to_limbs([o[4] for o in openings])),
            _ptr(_g1_limbs([o[5] for o in openings])), _ptr(_g1_limbs([o[6] for o in openings])),
            _ptr(ints_to_limbs(list(rhos))), ctypes.byref(ok)))
        return ok.value == 1

    # ---- KZG in evaluation form (include/pbf.h "KZG in evaluation form"; g1_ntt.hip, kzg_evals.hip)
    def ntt_g1(self, omega: int, points, inverse: bool = False) -> list:
        """pbf_ntt_g1_bn254: out[k] = sum_j [omega^(jk)] points[j] (the inverse: omega^-1 and
        n^-1); points as (x, y), the identity (0, 0). The points are checked on the curve."""
        n = len(points)
        out = np.zeros(8 * max(n, 1), dtype=np.uint64)
        _check(self.lib.pbf_ntt_g1_bn254(self.h, _ptr(ints_to_limbs([omega])), _ptr(_g1_limbs(points)), _ptr(out),
                                         n, int(inverse)))
        return self._points(out)[:n]

    def ntt_g1_dev(self, omega: int, d_in: int, d_out: int, n: int, inverse: bool = False, stream: int = 0) -> None:
        """The same on n device points (8 x u64 each, unchecked), enqueued on stream; d_in may be
        d_out."""
        _check(self.lib.pbf_ntt_g1_bn254_dev(self.h, _ptr(ints_to_limbs([omega])), _vp(d_in), _vp(d_out), n,
                                             int(inverse), _vp(stream) if stream else None))

    def ntt_g1_batch(self, omega: int, points, n: int, inverse: bool = False) -> list:
        """pbf_ntt_g1_bn254_batch: len(points) / n transforms of size n under one omega, transform b
        the points[b*n:(b+1)*n]; each is what ntt_g1 returns for that slice. Every point is checked."""
        batch = len(points) // n if n else 0
        if not n or batch * n != len(points):
            raise ValueError("points must hold whole transforms of size n")
        out = np.zeros(8 * max(len(points), 1), dtype=np.uint64)
        _check(self.lib.pbf_ntt_g1_bn254_batch(self.h, _ptr(ints_to_limbs([omega])), _ptr(_g1_limbs(points)),
                                               _ptr(out), n, batch, int(inverse)))
        return self._points(out)[:len(points)]

    def ntt_g1_batch_dev(self, omega: int, d_in: int, d_out: int, n: int, batch: int, inverse: bool = False,
                         stream: int = 0) -> None:
        """The same on batch x n device points (compact, unchecked), enqueued on stream; d_in may be
        d_out."""
        _check(self.lib.pbf_ntt_g1_bn254_batch_dev(self.h, _ptr(ints_to_limbs([omega])), _vp(d_in), _vp(d_out), n,
                                                   batch, int(inverse), _vp(stream) if stream else None))

    def srs_lagrange(self, srs, n: int, omega: int | None = None) -> list:
        """The Lagrange-basis SRS [L_i(s)]G, i < n, of srs = [s^j G]: the inverse G1 NTT of its
        first n points (no trapdoor). omega defaults to the library's root of unity of order n."""
        if n < 1 or n & (n - 1) or len(srs) < n:
            raise ValueError("n must be a power of two within the SRS")
        if omega is None:
            omega = pow(5, (BN254_R - 1) // n, BN254_R)  # fr_root_of_unity (csrc/fr_host.hpp)
        return self.ntt_g1(omega, list(srs[:n]), inverse=True)

    def kzg_open_evals(self, lsrs, omega: int, evals, z: int, weights, pitch: int | None = None):
        """pbf_kzg_open_evals_bn254: kzg_open for polynomials given by their n values on <omega>
        against the Lagrange-basis SRS: ([p_b(z)], W), the same W as kzg_open's."""
        a, n, pitch, batch = self._poly_limbs(evals, pitch)
        ys = np.zeros(4 * max(batch, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_evals_bn254(self.h, _ptr(_g1_limbs(lsrs[:n])), n, _ptr(ints_to_limbs([omega])),
                                                 _ptr(a), pitch, batch, _ptr(ints_to_limbs([z])),
                                                 _ptr(ints_to_limbs(list(weights))), _ptr(ys), _ptr(w)))
        return limbs_to_ints(ys)[:batch], self._points(w)[0]

    def kzg_open_evals_dev(self, d_lsrs: int, n: int, omega: int, d_evals: int, pitch: int, batch: int, z: int,
                           weights, stream: int = 0):
        ys = np.zeros(4 * max(batch, 1), dtype=np.uint64)
        w = np.zeros(8, dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_evals_bn254_dev(self.h, _vp(d_lsrs), n, _ptr(ints_to_limbs([omega])),
                                                     _vp(d_evals), pitch, batch, _ptr(ints_to_limbs([z])),
                                                     _ptr(ints_to_limbs(list(weights))), _ptr(ys), _ptr(w),
                                                     _vp(stream) if stream else None))
        return limbs_to_ints(ys)[:batch], self._points(w)[0]

    # ---- every opening at once (include/pbf.h "Every opening at once"; g1_mul.hip, kzg_cells.hip)
    def g1_mul(self, points, scalars) -> list:
        """pbf_g1_bn254_mul: [[k_i] P_i]; points as (x, y), the identity (0, 0). Points are
        checked on the curve and scalars < r."""
        n = len(scalars)
        if len(points) != n:
            raise ValueError("one scalar per point")
        out = np.zeros(8 * max(n, 1), dtype=np.uint64)
        _check(self.lib.pbf_g1_bn254_mul(self.h, _ptr(_g1_limbs(points)), _ptr(ints_to_limbs(list(scalars))),
                                         _ptr(out), n))
        return self._points(out)[:n]

    def g1_mul_dev(self, d_points: int, d_scalars: int, d_out: int, n: int, stream: int = 0) -> None:
        """The same on n device points and scalars (unchecked), enqueued on stream; d_out may be
        d_points."""
        _check(self.lib.pbf_g1_bn254_mul_dev(self.h, _vp(d_points), _vp(d_scalars), _vp(d_out), n,
                                             _vp(stream) if stream else None))

    def kzg_fk20_setup(self, srs, n: int, omega2: int) -> list:
        """pbf_kzg_fk20_setup_bn254: the 2n points xext of (srs, n) for omega2 of order 2n."""
        out = np.zeros(16 * max(n, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_fk20_setup_bn254(self.h, _ptr(_g1_limbs(srs) if len(srs) else np.zeros(8, np.uint64)),
                                                 len(srs), _ptr(ints_to_limbs([omega2])), n, _ptr(out)))
        return self._points(out)[:2 * n]

    def kzg_fk20_setup_dev(self, d_srs: int, srs_m: int, omega2: int, n: int, d_xext: int, stream: int = 0) -> None:
        _check(self.lib.pbf_kzg_fk20_setup_bn254_dev(self.h, _vp(d_srs), srs_m, _ptr(ints_to_limbs([omega2])), n,
                                                     _vp(d_xext), _vp(stream) if stream else None))

    def kzg_open_all(self, xext, omega2: int, polys, weights, pitch: int | None = None, with_y: bool = True):
        """pbf_kzg_open_all_bn254: every opening on <omega2^2> at once, n = len(xext) / 2:
        ([[p_b(omega^i)]] or None, [W_i]), each W_i the W of kzg_open at z = omega^i."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        n = len(xext) // 2
        ys = np.zeros(4 * max(batch * n, 1), dtype=np.uint64)
        w = np.zeros(8 * max(n, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_all_bn254(self.h, _ptr(_g1_limbs(xext)), n, _ptr(ints_to_limbs([omega2])),
                                               _ptr(a), ln, pitch, batch, _ptr(ints_to_limbs(list(weights))),
                                               _ptr(ys) if with_y else None, _ptr(w)))
        v = limbs_to_ints(ys)
        return ([v[b * n:(b + 1) * n] for b in range(batch)] if with_y else None), self._points(w)[:n]

    def kzg_open_all_dev(self, d_xext: int, n: int, omega2: int, d_polys: int, length: int, pitch: int, batch: int,
                         weights, d_out_y: int, d_out_w: int, stream: int = 0) -> None:
        """The same on the device: d_out_y (batch x n values, or 0 for none) and d_out_w (n points)
        are written on stream and stay there."""
        _check(self.lib.pbf_kzg_open_all_bn254_dev(self.h, _vp(d_xext), n, _ptr(ints_to_limbs([omega2])),
                                                   _vp(d_polys), length, pitch, batch,
                                                   _ptr(ints_to_limbs(list(weights))),
                                                   _vp(d_out_y) if d_out_y else None, _vp(d_out_w),
                                                   _vp(stream) if stream else None))

    # ---- cell proofs (include/pbf.h "KZG cell proofs"; kzg_cells.hip)
    def kzg_cells_setup(self, srs, n: int, l: int, omega2: int) -> list:
        """pbf_kzg_cells_setup_bn254: the 2n points xext of (srs, n, l), slab-major, for omega2 of
        order 2n."""
        out = np.zeros(16 * max(n, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_cells_setup_bn254(self.h, _ptr(_g1_limbs(srs) if len(srs) else np.zeros(8, np.uint64)),
                                                  len(srs), _ptr(ints_to_limbs([omega2])), n, l, _ptr(out)))
        return self._points(out)[:2 * n]

    def kzg_cells_setup_dev(self, d_srs: int, srs_m: int, omega2: int, n: int, l: int, d_xext: int,
                            stream: int = 0) -> None:
        _check(self.lib.pbf_kzg_cells_setup_bn254_dev(self.h, _vp(d_srs), srs_m, _ptr(ints_to_limbs([omega2])), n, l,
                                                      _vp(d_xext), _vp(stream) if stream else None))

    def kzg_open_cells(self, xext, l: int, omega2: int, polys, weights, pitch: int | None = None,
                       with_y: bool = True):
        """pbf_kzg_open_cells_bn254: one proof per cell of l points, n = len(xext) / 2, k = n / l:
        (ys or None, [W_i]) with ys[b][i] the l values p_b(omega^(i + k t)), t < l, of cell i."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        n = len(xext) // 2
        k = n // l if l else 0
        ys = np.zeros(4 * max(batch * n, 1), dtype=np.uint64)
        w = np.zeros(8 * max(k, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_cells_bn254(self.h, _ptr(_g1_limbs(xext)), n, l, _ptr(ints_to_limbs([omega2])),
                                                 _ptr(a), ln, pitch, batch, _ptr(ints_to_limbs(list(weights))),
                                                 _ptr(ys) if with_y else None, _ptr(w)))
        v = limbs_to_ints(ys)
        cells = [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)]
        return (cells if with_y else None), self._points(w)[:k]

    def kzg_open_cells_dev(self, d_xext: int, n: int, l: int, omega2: int, d_polys: int, length: int, pitch: int,
                           batch: int, weights, d_out_y: int, d_out_w: int, stream: int = 0) -> None:
        """The same on the device: d_out_y (batch x n values, cell-major, or 0 for none) and d_out_w
        (n / l points) are written on stream and stay there."""
        _check(self.lib.pbf_kzg_open_cells_bn254_dev(self.h, _vp(d_xext), n, l, _ptr(ints_to_limbs([omega2])),
                                                     _vp(d_polys), length, pitch, batch,
                                                     _ptr(ints_to_limbs(list(weights))),
                                                     _vp(d_out_y) if d_out_y else None, _vp(d_out_w),
                                                     _vp(stream) if stream else None))

    def kzg_open_cells_each(self, xext, l: int, omega2: int, polys, pitch: int | None = None, with_y: bool = True):
        """pbf_kzg_open_cells_each_bn254: the cell proofs of every polynomial in one call:
        (ys or None, ws) with ws[b] the k proofs kzg_open_cells gives for polynomial b alone under
        weight 1, and ys as kzg_open_cells returns it."""
        a, ln, pitch, batch = self._poly_limbs(polys, pitch)
        n = len(xext) // 2
        k = n // l if l else 0
        ys = np.zeros(4 * max(batch * n, 1), dtype=np.uint64)
        w = np.zeros(8 * max(batch * k, 1), dtype=np.uint64)
        _check(self.lib.pbf_kzg_open_cells_each_bn254(self.h, _ptr(_g1_limbs(xext)), n, l,
                                                      _ptr(ints_to_limbs([omega2])), _ptr(a), ln, pitch, batch,
                                                      _ptr(ys) if with_y else None, _ptr(w)))
        v = limbs_to_ints(ys)
        cells = [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)]
        pts = self._points(w)
        return (cells if with_y else None), [pts[b * k:(b + 1) * k] for b in range(batch)]

    def kzg_open_cells_each_dev(self, d_xext: int, n: int, l: int, omega2: int, d_polys: int, length: int, pitch: int,
                                batch: int, d_out_y: int, d_out_w: int, stream: int = 0) -> None:
        """The same on the device: d_out_y (batch x n values, cell-major, or 0 for none) and d_out_w
        (batch x n / l points, polynomial-major) are written on stream and stay there."""
        _check(self.lib.pbf_kzg_open_cells_each_bn254_dev(self.h, _vp(d_xext), n, l, _ptr(ints_to_limbs([omega2])),
                                                          _vp(d_polys), length, pitch, batch,
                                                          _vp(d_out_y) if d_out_y else None, _vp(d_out_w),
                                                          _vp(stream) if stream else None))

    def kzg_verify_cells(self, g2s, srs, omega: int, n: int, l: int, entries, rhos) -> bool:
        """pbf_kzg_verify_cells_bn254: g2s = [G2, [s^l]G2]; srs the first l points (or more);
        entries a list of (C, idx, ys, W) with ys the l values of cell idx; rhos the batching
        weights: nonzero, < r, chosen unpredictably after seeing the cells (soundness rests on
        that; include/pbf.h). One pairing check whatever the count."""
        if len(entries) != len(rhos):
            raise ValueError("one rho per entry")
        if any(len(e[2]) != l for e in entries):
            raise ValueError("l values per cell")
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_kzg_verify_cells_bn254(self.h, _ptr(_g2_limbs(g2s)), _ptr(_g1_limbs(srs)), len(srs),
                                                   _ptr(ints_to_limbs([omega])), n, l, len(entries),
                                                   _ptr(_g1_limbs([e[0] for e in entries])),
                                                   _ptr(_as_u64([e[1] for e in entries])),
                                                   _ptr(ints_to_limbs([v for e in entries for v in e[2]])),
                                                   _ptr(_g1_limbs([e[3] for e in entries])),
                                                   _ptr(ints_to_limbs(list(rhos))), ctypes.byref(ok)))
        return ok.value == 1

    # ---- recovery from cells (include/pbf.h "Recovery from cells"; kzg_recover.hip)
    def kzg_recover_cells(self, omega: int, n: int, l: int, length: int, cell_idx, cells, pitch: int | None = None,
                          with_y: bool = True):
        """pbf_kzg_recover_cells_bn254: cells[b][j] the l values of cell cell_idx[j] of polynomial b.
        (polys, ys or None, consistent): polys[b] the `length` coefficients, ys[b][i] the l values of
        cell i < n / l, consistent[b] 1 when the cells are those of a polynomial of `length`
        coefficients."""
        batch, count = len(cells), len(cell_idx)
        if any(len(c) != count for c in cells) or any(len(v) != l for c in cells for v in c):
            raise ValueError("one list of l values per known cell and polynomial")
        pitch = length if pitch is None else int(pitch)
        k = n // l if l else 0
        a = ints_to_limbs([v for c in cells for cell in c for v in cell]) if batch * count * l else np.zeros(4, np.uint64)
        out = np.zeros(4 * max(batch * max(pitch, length), 1), dtype=np.uint64)
        ys = np.zeros(4 * max(batch * n, 1), dtype=np.uint64)
        flags = np.zeros(max(batch, 1), dtype=np.int32)
        _check(self.lib.pbf_kzg_recover_cells_bn254(self.h, _ptr(ints_to_limbs([omega])), n, l, length, count,
                                                    _ptr(_as_u64(list(cell_idx) or [0])), _ptr(a), batch, _ptr(out),
                                                    pitch, _ptr(ys) if with_y else None,
                                                    flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        p, v = limbs_to_ints(out), limbs_to_ints(ys)
        polys = [p[b * pitch:b * pitch + length] for b in range(batch)]
        got = [[v[(b * k + i) * l:(b * k + i + 1) * l] for i in range(k)] for b in range(batch)]
        return polys, (got if with_y else None), [int(f) for f in flags[:batch]]

    def kzg_recover_cells_dev(self, omega: int, n: int, l: int, length: int, cell_idx, d_cells: int, batch: int,
                              d_out_polys: int, pitch: int, d_out_y: int, d_consistent: int, stream: int = 0) -> None:
        """The same on the device: d_out_polys (batch x pitch), d_out_y (batch x n values, cell-major,
        or 0 for none) and d_consistent (batch ints) are written on stream and stay there; cell_idx
        is a host list."""
        _check(self.lib.pbf_kzg_recover_cells_bn254_dev(self.h, _ptr(ints_to_limbs([omega])), n, l, length,
                                                        len(cell_idx), _ptr(_as_u64(list(cell_idx) or [0])),
                                                        _vp(d_cells), batch, _vp(d_out_polys), pitch,
                                                        _vp(d_out_y) if d_out_y else None, _vp(d_consistent),
                                                        _vp(stream) if stream else None))

    def plonk_prove_bn254_sharded_dev(self, comm: "Comm", n, d_q, d_copies, d_abc, chal, rnd, d_srs, srs_m,
                                      k1k2=(2, 3), mode=0, stream: int = 0):
        """This rank's part of the multi-GPU prove (include/pbf.h); comm: a Comm struct."""
        pts = np.zeros(72, dtype=np.uint64)
        fs = np.zeros(28, dtype=np.uint64)
        _check(self.lib.pbf_plonk_prove_bn254_sharded_dev(self.h, ctypes.addressof(comm), n, d_q, d_copies, d_abc,
                                                          _ptr(ints_to_limbs(chal)), _ptr(ints_to_limbs(rnd)),
                                                          _ptr(ints_to_limbs(k1k2)), d_srs, srs_m, mode, _ptr(pts),
                                                          _ptr(fs), stream))
        return pts, fs

    # ---- plonk-by-hand types (src/pbh/*.rs), batched on the GPU
    def _u32call(self, fn, a, b, width_out, n):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(b, dtype=np.uint32).reshape(-1))
        out = np.zeros(n * width_out, dtype=np.uint32)
        _check(fn(self.h, a.ctypes.data_as(_p32), b.ctypes.data_as(_p32), n, out.ctypes.data_as(_p32)))
        return [tuple(int(x) for x in out[i * width_out:(i + 1) * width_out]) for i in range(n)]

    # ---- BN254 pairing (config 4 pairing check; pairing.hip)
    def pairing_bn254(self, g1s, g2s) -> np.ndarray:
        """[(x, y)] G1 affine and [((x0, x1), (y0, y1))] G2 affine (None = identity) ->
        n x 12 Fq ints (tower order c0.a0.re, c0.a0.im, ..., c1.a2.im)."""
        n = len(g1s)
        a = _g1_limbs(g1s)
        b = _g2_limbs(g2s)
        out = np.zeros(n * 48, dtype=np.uint64)
        _check(self.lib.pbf_pairing_bn254(self.h, _ptr(a), _ptr(b), n, _ptr(out)))
        return [limbs_to_ints(out[48 * i: 48 * (i + 1)]) for i in range(n)]

    def pairing_bn254_dev(self, d_g1: int, d_g2: int, n: int, d_out: int, stream: int = 0) -> None:
        _check(self.lib.pbf_pairing_bn254_dev(self.h, d_g1, d_g2, n, d_out, stream))

    def pairing_check_bn254(self, g1s, g2s) -> bool:
        a = _g1_limbs(g1s)
        b = _g2_limbs(g2s)
        ok = ctypes.c_int(-1)
        _check(self.lib.pbf_pairing_check_bn254(self.h, _ptr(a), _ptr(b), len(g1s), ctypes.byref(ok)))
        return ok.value == 1

    def g2_bn254_mul(self, pts, scalars) -> list:
        n = len(pts)
        a = _g2_limbs(pts)
        s = ints_to_limbs([int(x) for x in scalars])
        out = np.zeros(n * 16, dtype=np.uint64)
        _check(self.lib.pbf_g2_bn254_mul(self.h, _ptr(a), _ptr(s), n, _ptr(out)))
        res = []
        for i in range(n):
            v = limbs_to_ints(out[16 * i: 16 * (i + 1)])
            res.append(None if not any(v) else ((v[0], v[1]), (v[2], v[3])))
        return res

    def pbh_g1_mul(self, pts, scalars):
        return self._u32call(self.lib.pbf_pbh_g1_mul, pts, scalars, 3, len(scalars))

    def pbh_g2_mul(self, pts, scalars):
        return self._u32call(self.lib.pbf_pbh_g2_mul, pts, scalars, 2, len(scalars))

    def pbh_gt_pow(self, xs, es):
        return self._u32call(self.lib.pbf_pbh_gt_pow, xs, es, 2, len(es))

    def pbh_pairing(self, g1s, g2s):
        return self._u32call(self.lib.pbf_pbh_pairing, g1s, g2s, 2, len(g2s))

    def pbh_prove(self, gates, copies, abc, chal, rnd, s=2, srs_n=6, omega_pows=4, verify_u=None):
        """Plonk::prove (+verify) over PlonkByHandTypes; same layout as oracle.pbh_prove."""
        n = len(gates)
        a = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.uint64).reshape(-1))  # noqa: E731
        g, c, w = a(gates), a(copies), a(abc)
        ch, rd = a(chal), a(rnd)
        pts = np.zeros(27, np.uint64)
        fs = np.zeros(7, np.uint64)
        ver = ctypes.c_int()
        _check(self.lib.pbf_pbh_prove(self.h, n, _ptr(g), _ptr(c), _ptr(w), _ptr(ch), _ptr(rd), s, srs_n,
                                      omega_pows, 17 if verify_u is None else verify_u, _ptr(pts), _ptr(fs),
                                      ctypes.byref(ver)))
        points = [tuple(int(x) for x in pts[3 * i: 3 * i + 3]) for i in range(9)]
        return points, [int(x) for x in fs], (None if verify_u is None else bool(ver.value))

    def fill_random_dev(self, modulus: int, seed: int, d_out: int, count: int, stream: int = 0) -> None:
        _check(self.lib.pbf_fill_random_u64_dev(self.h, modulus, seed, _vp(d_out), count,
                                                _vp(stream) if stream else None))


Q32 = 3221225473  # 3 * 2^30 + 1 (the reference-literal cross-check prime)


class Comm(ctypes.Structure):
    """struct pbf_comm (include/pbf.h): world, rank, user, send, recv, capacity and the
    all_to_all / all_gather callbacks (CFUNCTYPE(c_int, c_void_p, c_size_t, c_void_p))."""

    _fields_ = [("world", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("user", ctypes.c_void_p),
                ("send", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("capacity", ctypes.c_size_t),
                ("all_to_all", ctypes.c_void_p), ("all_gather", ctypes.c_void_p)]

    def __init__(self, world, rank, send, recv, capacity, a2a, ag):
        super().__init__(world, rank, None, send, recv, capacity, ctypes.cast(a2a, ctypes.c_void_p),
                         ctypes.cast(ag, ctypes.c_void_p))


def default_root(modulus: int):
    """(root, log2 of its order) of a maximal 2-power root of unity for the supported NTT
    primes: Goldilocks (generator 7, 2-adicity 32) and q32 (generator 5, 2-adicity 30)."""
    if modulus == GOLDILOCKS:
        return pow(7, (modulus - 1) >> 32, modulus), 32
    if modulus == Q32:
        return pow(5, (modulus - 1) >> 30, modulus), 30
    raise ValueError("pass root and root_log for this modulus")


BN254_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN254_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def _circuit_limbs(q, copies, srs, abc=None):
    """The limb arrays of a host circuit and SRS, (qa, ca, sa) or with a witness (qa, ca, aa, sa): q 5
    columns of ints, copies 3 columns of (kind, 1-based idx), abc 3 columns, srs affine points."""
    qa = ints_to_limbs([x for col in q for x in col])
    ca = np.array([v for col in copies for (k, i) in col for v in (k, i)], dtype=np.uint64)
    sa = _g1_limbs(srs)
    return (qa, ca, sa) if abc is None else (qa, ca, ints_to_limbs([x for col in abc for x in col]), sa)


def _proof_limbs(pts, fields):
    """(72, 28) u64 limbs of a proof given as the provers return it: limb arrays, or points and ints."""
    pa = pts if isinstance(pts, np.ndarray) else _g1_limbs(pts)
    fa = fields if isinstance(fields, np.ndarray) else ints_to_limbs(fields)
    return np.ascontiguousarray(pa, dtype=np.uint64), np.ascontiguousarray(fa, dtype=np.uint64)


def _g1_limbs(pts) -> np.ndarray:
    return ints_to_limbs([c for p in pts for c in ((0, 0) if p is None else p)])


def _g2_limbs(pts) -> np.ndarray:
    return ints_to_limbs([c for p in pts for c in ((0, 0, 0, 0) if p is None else (p[0][0], p[0][1], p[1][0], p[1][1]))])


def kzg_fold(commits, ys, weights, ctx: "Context | None" = None):
    """A batched opening as one verifier entry: (sum_b w_b C_b, sum_b w_b y_b mod r) for the
    commitments C_b, claimed evaluations y_b and the opening's weights w_b; with the opening's z
    and W it is one (C, z, y, W) entry of Context.kzg_verify. The point sum is an MSM (msm_g1)."""
    if not (len(commits) == len(ys) == len(weights)):
        raise ValueError("one evaluation and one weight per commitment")
    c = (ctx or default_context()).msm_g1(list(commits), [int(w) % BN254_R for w in weights])
    return c, sum(int(w) * int(y) for w, y in zip(weights, ys)) % BN254_R


def ints_to_limbs(values) -> np.ndarray:
    """Python ints -> flat array of 4 x u64 little-endian limbs per element."""
    out = np.empty(len(values) * 4, dtype=np.uint64)
    m = (1 << 64) - 1
    for i, v in enumerate(values):
        v = int(v)
        out[4 * i: 4 * i + 4] = [v & m, (v >> 64) & m, (v >> 128) & m, (v >> 192) & m]
    return out


def limbs_to_ints(a: np.ndarray) -> list:
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a]


# ---- multi-GPU from one process (pbf_*_multi): a list of Contexts, rank g = ctxs[g] -----------
def _ctx_array(ctxs):
    arr = (_vp * len(ctxs))(*[c.h for c in ctxs])
    return arr, len(ctxs)


def _ptr_array(ptrs):
    return (_vp * len(ptrs))(*[_vp(p) if p else None for p in ptrs])


def multi_backend(ctxs) -> str:
    arr, w = _ctx_array(ctxs)
    b = ctypes.c_int(-1)
    _check(load_library().pbf_multi_backend(arr, w, ctypes.byref(b)))
    return {0: "device-copies", 1: "rccl"}[b.value]


def ntt_multi(ctxs, modulus: int, omega: int, values, inverse: bool = False) -> np.ndarray:
    """pbf_ntt_u64_multi: fft.rs:66-78 of one vector with its top log2(G) levels across the ranks."""
    arr, w = _ctx_array(ctxs)
    a = _as_u64(values)
    out = np.empty_like(a)
    _check(load_library().pbf_ntt_u64_multi(arr, w, modulus, omega, _ptr(a), _ptr(out), a.size, int(inverse)))
    return out


def ntt_multi_dev(ctxs, modulus: int, omega: int, d_in, d_out, nl: int, batch: int, inverse: bool = False,
                  streams=None) -> None:
    arr, w = _ctx_array(ctxs)
    _check(load_library().pbf_ntt_u64_multi_dev(arr, w, modulus, omega, _ptr_array(d_in), _ptr_array(d_out), nl, batch,
                                                int(inverse), _ptr_array(streams) if streams else None))


def ntt_fr_multi(ctxs, omega: int, values, inverse: bool = False) -> list:
    arr, w = _ctx_array(ctxs)
    a = ints_to_limbs(values)
    out = np.empty_like(a)
    _check(load_library().pbf_ntt_fr256_multi(arr, w, _ptr(ints_to_limbs([omega])), _ptr(a), _ptr(out), len(values),
                                              int(inverse)))
    return limbs_to_ints(out)


def mul_ntt_multi(ctxs, modulus: int, omega: int, a, b) -> np.ndarray:
    arr, w = _ctx_array(ctxs)
    a = _as_u64(a)
    b = _as_u64(b)
    out = np.empty(a.size + b.size, dtype=np.uint64)
    _check(load_library().pbf_mul_ntt_u64_multi(arr, w, modulus, omega, _ptr(a), a.size, _ptr(b), b.size, _ptr(out)))
    return out


def mul_ntt_fr_multi(ctxs, omega: int, a, b) -> list:
    arr, w = _ctx_array(ctxs)
    al, bl = ints_to_limbs(a), ints_to_limbs(b)
    out = np.empty((len(a) + len(b)) * 4, dtype=np.uint64)
    _check(load_library().pbf_mul_ntt_fr256_multi(arr, w, _ptr(ints_to_limbs([omega])), _ptr(al), len(a), _ptr(bl),
                                                  len(b), _ptr(out)))
    return limbs_to_ints(out)


def plonk_prove_bn254_multi(ctxs, q, copies, abc, chal, rnd, srs, k1k2=(2, 3), mode=1):
    """pbf_plonk_prove_bn254_multi (host inputs; same conventions as Context.plonk_prove_bn254)."""
    arr, w = _ctx_array(ctxs)
    n = len(abc[0])
    qa, ca, aa, sa = _circuit_limbs(q, copies, srs, abc)
    pts = np.zeros(72, dtype=np.uint64)
    fs = np.zeros(28, dtype=np.uint64)
    _check(load_library().pbf_plonk_prove_bn254_multi(arr, w, n, _ptr(qa), _ptr(ca), _ptr(aa), _ptr(ints_to_limbs(chal)),
                                                      _ptr(ints_to_limbs(rnd)), _ptr(ints_to_limbs(k1k2)), _ptr(sa),
                                                      len(srs), mode, _ptr(pts), _ptr(fs)))
    pv = limbs_to_ints(pts)
    return [None if pv[2 * i] == 0 and pv[2 * i + 1] == 0 else (pv[2 * i], pv[2 * i + 1]) for i in range(9)], \
        limbs_to_ints(fs)


def plonk_prove_bn254_multi_dev(ctxs, n, d_q, d_copies, d_abc, chal, rnd, d_srs, srs_m, k1k2=(2, 3), mode=1,
                                streams=None):
    """pbf_plonk_prove_bn254_multi_dev: per-rank device inputs (lists of pointers); returns the
    proof as limb arrays (9 x 8 u64 points, 7 x 4 u64 fields)."""
    arr, w = _ctx_array(ctxs)
    pts = np.zeros(72, dtype=np.uint64)
    fs = np.zeros(28, dtype=np.uint64)
    _check(load_library().pbf_plonk_prove_bn254_multi_dev(
        arr, w, n, _ptr_array(d_q), _ptr_array(d_copies), _ptr_array(d_abc), _ptr(ints_to_limbs(chal)),
        _ptr(ints_to_limbs(rnd)), _ptr(ints_to_limbs(k1k2)), _ptr_array(d_srs), srs_m, mode, _ptr(pts), _ptr(fs),
        _ptr_array(streams) if streams else None))
    return pts, fs


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---- the reference's FFT trait surface (fft.rs:6-21) ------------------------
class EvaluationDomainGenerator:
    """fft.rs:6-15"""

    def __init__(self, omega: int, size: int):
        self.omega = int(omega)
        self.size = int(size)


class CooleyTurkey:
    """FFT<F> for U64Field<modulus> on the GPU (fft.rs:51-79). `fft` and
    `fft_inv` take and return canonical residues, natural order."""

    def __init__(self, modulus: int, domain: EvaluationDomainGenerator, ctx: Context | None = None):
        self.modulus = int(modulus)
        self.domain = domain
        self.ctx = ctx or default_context()

    @classmethod
    def new(cls, modulus: int, domain: EvaluationDomainGenerator, ctx: Context | None = None) -> "CooleyTurkey":
        return cls(modulus, domain, ctx)

    def fft(self, values) -> np.ndarray:
        return self.ctx.ntt(self.modulus, self.domain.omega, values, inverse=False)

    def fft_inv(self, freq) -> np.ndarray:
        return self.ctx.ntt(self.modulus, self.domain.omega, freq, inverse=True)

    def coset_fft(self, values, shift: int, n: int | None = None) -> np.ndarray:
        """Evaluations of the polynomial `values` on shift * <omega_n> (n: the domain size, default
        len(values); a larger power of two needs the matching `domain`): a low-degree extension."""
        return self.ctx.ntt_coset(self.modulus, self.domain.omega, shift, values, n=n)

    def coset_fft_inv(self, freq, shift: int) -> np.ndarray:
        return self.ctx.ntt_coset(self.modulus, self.domain.omega, shift, freq, inverse=True)


def mul_ntt(fft: CooleyTurkey, a_vals, b_vals) -> np.ndarray:
    """fft.rs:109-132: length la+lb, not normalised."""
    return fft.ctx.mul_ntt(fft.modulus, fft.domain.omega, a_vals, b_vals)


def normalize(coeffs: np.ndarray) -> np.ndarray:
    """poly.rs:96-105 Poly::new normalisation (strip trailing zeros, keep one)."""
    c = np.asarray(coeffs, dtype=np.uint64)
    nz = np.nonzero(c)[0]
    return c[: (nz[-1] + 1 if nz.size else 1)].copy()
