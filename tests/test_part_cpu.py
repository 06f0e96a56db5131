"""The device partition's host side (CPU only): the header declares the calls
and names the reference seams, the ctypes table binds each with the argument
count of its prototype, the wrapper has the methods, and the pack-map host step
(parmmg_amd/csrc/pmx_part_pack.h) equals the CPU twin's numbering -- a
stand-alone program under ASan / UBSan (tests/c/part_pack_asan.cpp)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "c", "_build")
SAN = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CALLS = {"pmx_part_from_marks": 5, "pmx_part_upload": 3, "pmx_part_download": 3, "pmx_part_fix": 3,
         "pmx_split_groups_part": 6, "pmx_part_release": 1}


def header():
    with open(os.path.join(ROOT, "include", "pmx_transfer.h"), encoding="utf-8") as fh:
        return fh.read()


def test_header_declares_and_bindings_bind_the_calls():
    from parmmg_amd import _native as N
    hdr = header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in CALLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name}: no prototype"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs and params[0] == "pmx_ctx *ctx", name
        restype, argtypes = N.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs and argtypes[0] is C.c_void_p, name
        # a pointer parameter is bound as a pointer, a scalar as a scalar
        for p, a in zip(params[1:], argtypes[1:]):
            assert ("*" in p) == (a is C.c_void_p or issubclass(a, C._Pointer)), (name, p)
    assert "PMMG_part_getInterfaces (src/moveinterfaces_pmmg.c:1150-1212)" in hdr
    assert "pmx_part_from_marks / _upload" in hdr and "which = 24" in hdr


def test_wrapper_has_the_methods():
    from parmmg_amd.transfer import Transfer
    for name in ("part_from_marks", "part_upload", "part_download", "part_fix", "split_groups_part", "part_release"):
        assert callable(getattr(Transfer, name)), name


def test_the_source_is_built_and_names_its_threshold():
    from parmmg_amd import build
    assert "pmx_part.hip" in build.HIP_SOURCES
    with open(os.path.join(ROOT, "parmmg_amd", "csrc", "pmx_part.hip"), encoding="utf-8") as fh:
        src = fh.read()
    assert re.search(r"^#define PT_LDS_COLOURS \d+", src, re.M)
    assert "getenv" not in src


def test_pack_map_equals_the_twin_under_asan_ubsan():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "part_pack_asan")
    cmd = ["g++", "-Wall", *SAN, "-I", os.path.join(ROOT, "parmmg_amd", "csrc"),
           "-x", "c++", os.path.join(ROOT, "tests", "c", "part_pack_asan.cpp"),
           "-x", "c", os.path.join(ROOT, "tests", "c", "moveifc_ref.c"), "-o", exe, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "part pack asan ok" in r.stdout
