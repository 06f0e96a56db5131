"""ASan/UBSan build of the reachability check's CPU twin (tests/c/reach_ref.c)
with the mesh generator, driven by the stand-alone tests/c/reach_asan.c (CPU):
leaks, out-of-bounds accesses and undefined behaviour fail the test."""
import os
import subprocess

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "c", "_build")
SAN = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_reach_twin_under_asan_ubsan():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "reach_asan")
    srcs = [os.path.join(ROOT, "tests", "c", f) for f in ("reach_asan.c", "reach_ref.c")]
    srcs.append(os.path.join(ROOT, "parmmg_amd", "csrc", "meshgen.c"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", *SAN, *srcs, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reach asan ok" in r.stdout
