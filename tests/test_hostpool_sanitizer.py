"""ThreadSanitizer build of the host thread pool (parmmg_amd/csrc/pmx_hostpool.hip,
plain C++: compiled here as ``-x c++``), driven by the stand-alone
tests/c/hostpool_tsan.cpp (CPU): a data race or a range element visited any
other number of times than once fails the test.  Every host packing pass of
the library runs on this pool, and PMX_interpMetricsAndFields enters it from
two threads."""
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "c", "_build")
CSRC = os.path.join(ROOT, "parmmg_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=thread"]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "hostpool_tsan")
    cmd = ["g++", *SAN, "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "c", "hostpool_tsan.cpp"),
           "-x", "c++", os.path.join(CSRC, "pmx_hostpool.hip"), "-o", out, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


# 1000: ranges on both sides of the serial threshold; 1: a range shorter than
# the thread count is split too, so that some of its chunks are empty
@pytest.mark.parametrize("serial_below", ["1000", "1"])
def test_host_pool_under_tsan(exe, serial_below):
    env = dict(os.environ, PMX_HOST_THREADS="6", PMX_HOST_THREADS_MIN=serial_below,
               TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "threads 6, serial below " + serial_below in r.stdout
    assert "hostpool tsan ok" in r.stdout
