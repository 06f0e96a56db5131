"""Device memory, pinned memory and events are allocated and released in one
place, csrc/pmx_host.h (DevBuf / PinBuf / DevEvent): a raw call anywhere else
fails here.  The one exception is the memory pmx_device_alloc hands to the
caller, which pmx_device_free takes back."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parmmg_amd", "csrc")
OWNER = "pmx_host.h"

RAW_CALLS = ["hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreate", "hipEventDestroy"]
# file -> function -> the raw calls its body may hold
ALLOWED = {"pmx_capi.hip": {"pmx_device_alloc": {"hipMalloc(": 1, "hipFree(": 1},   # the free: its memset failed
                            "pmx_device_free": {"hipFree(": 1}}}
GONE = ["free_all", "sp_free", "dfree(", "MCK(", "struct Scratch"]
# files whose host code checks every HIP call through the call helper
# (pmx_host.h: pmx_call, PMX_CK): no comparison with hipSuccess by hand.
# pmx_capi.hip is not among them: pmx_create has no context to report to yet,
# and pmx_device_free reports a failed free through its return value alone.
ON_CALL_HELPER = ["pmx_quality.hip", "pmx_lengths.hip", "pmx_graph.hip", "pmx_reduce.hip",
                  "pmx_bdy.hip", "pmx_fans.hip", "pmx_seq.hip",
                  "pmx_points.hip", "pmx_results.hip", "pmx_hostpool.hip"]


def _sources():
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            yield f, fh.read()


def _count(text, call):
    # "hipMalloc(" must not count inside "hipHostMalloc(" and the like
    return len(re.findall(r"(?<![A-Za-z0-9_])" + re.escape(call), text))


def _body(text, func):
    """The definition of the extern "C" function `func`: from its header at
    the start of a line to the closing brace at the start of a line."""
    m = re.search(r"^[\w \*]*\b" + func + r"\([^;{]*\)\s*\{\n.*?^\}\n", text, re.S | re.M)
    assert m, f"{func}: definition not found"
    return m.group(0)


def test_raw_calls_only_in_the_owner():
    seen = 0
    for f, text in _sources():
        if f == OWNER:
            seen = sum(_count(text, c) for c in RAW_CALLS)
            continue
        allowed = {c: 0 for c in RAW_CALLS}
        for func, calls in ALLOWED.get(f, {}).items():
            body = _body(text, func)
            for c in RAW_CALLS:
                assert _count(body, c) == calls.get(c, 0), (f, func, c)
                allowed[c] += calls.get(c, 0)
        for c in RAW_CALLS:
            assert _count(text, c) == allowed[c], f"{f}: {c} outside {OWNER}"
    assert seen >= len(RAW_CALLS), f"{OWNER} holds no allocation sites: the scan is broken"


def test_owner_has_one_site_per_call():
    text = dict(_sources())[OWNER]
    for c in RAW_CALLS:
        assert _count(text, c) == 1, c


def test_hand_kept_lists_are_gone():
    for f, text in _sources():
        for word in GONE:
            assert word not in text, f"{f}: {word}"


def test_converted_files_hold_no_hand_checks():
    texts = dict(_sources())
    for f in ON_CALL_HELPER:
        assert f in texts, f"{f}: no such file (renamed? keep the list in step)"
        assert "hipSuccess" not in texts[f], f"{f}: a hand-written hipSuccess check"
