"""A kernel sits beside the host code that launches it: csrc/pmx_kernels.h
declares a launch_* function only when a source file other than the one that
defines it calls it.  A launcher with a single calling file is static in that
file, and there is no source left that is named for nothing."""
import os
import re

from parmmg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parmmg_amd", "csrc")
HEADER = "pmx_kernels.h"


def _code(name):
    """The file's text without its // comments."""
    with open(os.path.join(CSRC, name), encoding="utf-8") as fh:
        return re.sub(r"//[^\n]*", "", fh.read())


def _declared():
    names = re.findall(r"^[\w \*]*\b(launch_\w+)\([^;{]*\);", _code(HEADER), re.M)
    assert len(names) >= 10, f"{HEADER}: {len(names)} launchers found: the scan is broken"
    assert len(set(names)) == len(names), names
    return names


def _sources():
    return {f: _code(f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")}


def _defining(name, sources):
    """The files that define `name`: its header at the start of a line, a body after it."""
    pat = re.compile(r"^[\w \*]*\b" + name + r"\([^;{]*\)\s*\{", re.M)
    return [f for f, text in sources.items() if pat.search(text)]


def test_declared_launchers_are_defined_once():
    sources = _sources()
    for name in _declared():
        assert len(_defining(name, sources)) == 1, (name, _defining(name, sources))


def test_declared_launchers_are_called_from_another_file():
    sources = _sources()
    alone = []
    for name in _declared():
        home = _defining(name, sources)
        if not any(re.search(r"\b" + name + r"\(", text) for f, text in sources.items() if f not in home):
            alone.append((name, home))
    assert not alone, f"declared in {HEADER}, called only where defined (make them static): {alone}"


def test_no_source_named_for_nothing():
    assert "pmx_kernels.hip" not in build.HIP_SOURCES
    assert not os.path.exists(os.path.join(CSRC, "pmx_kernels.hip"))
