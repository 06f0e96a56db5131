"""CPU: the point-map seam of integration/pmmg_pmx.c and its constants.

A ParMmg built with USE_POINTMAP hands every new point's source vertex
(MMG5_Point.src) to the device path; without the macro the adapter is what it
was.  Both compile as C99 with -Wall -Wextra -Werror, each against its own
test-local parmmg.h (tests/c/pmmg_stub_pointmap/ has MMG5_Point.src).
"""
import os
import re
import subprocess

from conftest import ROOT
from parmmg_amd import _native as N

ADAPTER = os.path.join(ROOT, "integration", "pmmg_pmx.c")
HEADER = os.path.join(ROOT, "include", "pmx_transfer.h")


def _compile(tmp_path, stub, *defs):
    out = os.path.join(str(tmp_path), "pmmg_pmx_" + stub + ".o")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", *defs, "-c",
                    "-I", os.path.join(ROOT, "tests", "c", stub), "-I", os.path.join(ROOT, "include"),
                    ADAPTER, "-o", out], check=True)
    syms = subprocess.run(["nm", "-u", out], check=True, capture_output=True, text=True).stdout
    return set(line.split()[-1] for line in syms.splitlines() if line.strip())


def test_adapter_compiles_with_pointmap(tmp_path):
    und = _compile(tmp_path, "pmmg_stub_pointmap", "-DUSE_POINTMAP")
    assert "PMX_interpMetricsAndFields_groups_src" in und
    assert "PMX_interpMetricsAndFields_groups" not in und


def test_adapter_without_pointmap_is_unchanged(tmp_path):
    und = _compile(tmp_path, "pmmg_stub")
    assert "PMX_interpMetricsAndFields_groups" in und
    assert "PMX_interpMetricsAndFields_groups_src" not in und
    # and the macro cannot be honoured by a Mmg without the point map
    r = subprocess.run(["gcc", "-std=c99", "-DUSE_POINTMAP", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "c", "pmmg_stub"), "-I", os.path.join(ROOT, "include"),
                        ADAPTER], capture_output=True, text=True)
    assert r.returncode != 0 and "src" in r.stderr


def test_run_pointmap_matches_header():
    text = open(HEADER).read()
    flags = {name: int(val, 16) for name, val in re.findall(r"#define\s+PMX_RUN_(\w+)\s+(0x[0-9a-fA-F]+)", text)}
    assert flags["POINTMAP"] == 0x200 == N.RUN_POINTMAP
    others = [v for k, v in flags.items() if k != "POINTMAP"]
    assert all(v & 0x200 == 0 for v in others)
    for sym in ("pmx_upload_point_sources", "PMX_interpMetricsAndFields_groups_src", "pmx_pointmap_stats"):
        assert sym in N.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", text)
    assert [f for f, _ in N.PointSources._fields_] == ["src", "stride"]
