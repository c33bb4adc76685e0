"""The C-ABI library builds, loads and exports every symbol include/pbf.h declares
(CPU only: no compute calls are made without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pbf.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pbf_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    for must in ("pbf_ctx_create", "pbf_ntt_u64", "pbf_ntt_u64_batch_dev", "pbf_mul_ntt_u64", "pbf_poly_eval_u64"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    import pbf

    lib = pbf.load_library()
    for s in declared_symbols():
        assert hasattr(lib, s), s
    # the Python binding describes every declared entry point
    assert sorted(n for n, _, _ in pbf.SIGNATURES) == declared_symbols()


def test_exported_symbols_have_c_linkage():
    import pbf

    out = subprocess.run(["nm", "-D", "--defined-only", pbf.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (pbf_[a-z0-9_]+)", out.stdout))
    assert set(declared_symbols()) <= exported


def test_library_does_not_link_the_oracle():
    import pbf

    out = subprocess.run(["nm", "-D", pbf.LIB_PATH], capture_output=True, text=True, check=True)
    assert "oracle_" not in out.stdout
    ldd = subprocess.run(["ldd", pbf.LIB_PATH], capture_output=True, text=True).stdout
    assert "liboracle" not in ldd


def test_missing_library_fails_loudly(tmp_path):
    import pbf

    saved = pbf._lib
    pbf._lib = None
    try:
        with pytest.raises(ImportError):
            pbf.load_library(str(tmp_path / "nope.so"))
    finally:
        pbf._lib = saved


def test_last_error_callable_without_gpu():
    import pbf

    lib = pbf.load_library()
    assert isinstance(lib.pbf_last_error(), (bytes, type(None)))
    h = ctypes.c_void_p()
    rc = lib.pbf_ctx_create(-1, ctypes.byref(h))
    assert rc != 0  # invalid device index (or no device here) is an error code, not a crash


def test_single_hip_runtime_in_process():
    import pbf

    pbf.load_library()
    maps = open("/proc/self/maps").read()
    paths = {line.split()[-1] for line in maps.splitlines() if "libamdhip64" in line}
    assert len(paths) == 1, paths


def test_product_library_reads_no_tuning_environment():
    """the library never takes a schedule or a code path from the
    environment -- tuning goes through pbf_ctx_set_option (include/pbf.h), and there is no build
    that reads switches of alternative variants from it either. The only variable names in
    libpbf.so, and the only getenv calls in csrc/, are the RCCL library path and the
    single-device test hook of the RCCL branch (csrc/group.hip)."""
    import pbf

    data = open(pbf.LIB_PATH, "rb").read()
    names = set(re.findall(rb"PBF_[A-Z0-9_]{3,}", data))
    assert names <= {b"PBF_RCCL_LIB", b"PBF_GROUP_FORCE_RCCL"}, sorted(names)
    calls = []
    for fn, text in sorted(csrc_sources().items()):
        calls += [(fn, m) for m in re.findall(r"getenv\s*\(\s*([^)]*?)\s*\)", text)]
    assert calls == [("group.hip", '"PBF_RCCL_LIB"'), ("group.hip", '"PBF_GROUP_FORCE_RCCL"')], calls


def csrc_sources():
    """csrc/*.hip and *.hpp by file name, comments blanked out (line structure kept)."""
    src = os.path.join(ROOT, "plonk-by-fingers_amd", "csrc")
    blank = lambda m: re.sub(r"[^\n]", " ", m.group(0))
    out = {}
    for fn in os.listdir(src):
        if fn.endswith((".hip", ".hpp")):
            text = open(os.path.join(src, fn)).read()
            out[fn] = re.sub(r"//[^\n]*|/\*.*?\*/", blank, text, flags=re.S)
    return out


def kernel_definitions(text):
    """(name, offset of the name) of every __global__ function declared in `text`: the first
    identifier after `__global__ void` that is not a launch-bound or attribute clause."""
    found = []
    for m in re.finditer(r"\b__global__\b", text):
        i = m.end()
        while True:
            t = re.compile(r"\s*(\w+)").match(text, i)
            assert t, text[m.start():m.start() + 120]
            word, i = t.group(1), t.end()
            if word in ("void", "static", "inline"):
                continue
            if word not in ("__launch_bounds__", "__attribute__"):
                found.append((word, t.start(1)))
                break
            depth = 0  # skip the clause's balanced parentheses
            while True:
                depth += {"(": 1, ")": -1}.get(text[i], 0)
                i += 1
                if depth == 0 and text[i - 1] == ")":
                    break
    return found


def test_every_kernel_has_a_launch():
    """A __global__ function that nothing in csrc/ names outside its own declaration (and
    outside comments) cannot run in the shipped library: it is dead code that still costs build
    time and review. Kernels are launched by name here (directly or through a function-pointer
    selection that names them), so a plain search decides it."""
    sources = csrc_sources()
    kernels = []
    for fn, text in sources.items():
        kernels += [(fn, name, at) for name, at in kernel_definitions(text)]
    assert len(kernels) > 100, len(kernels)  # the search itself found the kernels
    declared = {(fn, at) for fn, _, at in kernels}
    unlaunched = []
    for fn, name, _ in kernels:
        uses = [(f, m.start()) for f, text in sources.items() for m in re.finditer(r"\b%s\b" % name, text)]
        if not [u for u in uses if u not in declared]:
            unlaunched.append((fn, name))
    assert not unlaunched, unlaunched


def test_no_build_switches_in_csrc():
    """The library has one build. The only preprocessor conditionals in csrc/ tell the host pass
    of a translation unit from the device pass (__HIP_DEVICE_COMPILE__); a macro that selects a
    timing mode or overrides a tuned constant (the retired PBF_GL_NOMATH, PBF_RS_ITEMS, ...)
    would be a second build that no test compiles."""
    found = []
    for fn, text in sorted(csrc_sources().items()):
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)", text, flags=re.M):
            found.append((fn, m.group(1).strip()))
    assert len(found) >= 4, found  # the search itself found the host / device conditionals
    allowed = ("__HIP_DEVICE_COMPILE__", "defined(__HIP_DEVICE_COMPILE__)")
    assert [f for f in found if f[1] not in allowed] == []


def test_set_option_is_declared_with_its_names():
    src = open(HEADER).read()
    assert "pbf_ctx_set_option" in src
    capi = open(os.path.join(ROOT, "plonk-by-fingers_amd", "csrc", "capi.hip")).read()
    known = re.search(r"known\[\] = \{(.*?)\};", capi, flags=re.S).group(1)
    for name in re.findall(r"\"([a-z0-9_.]+)\"", known):
        assert name in src, name  # every accepted option is documented in pbf.h
