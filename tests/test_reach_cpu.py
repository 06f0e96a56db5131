"""The CPU twin of the reachability check (tests/c/reach_ref.c) on the cases
the GPU tests compare against (CPU only): its fix is the contiguity twin's, the
flags the fix leaves are a function of the fixed marks, the counter ends at ne
on a connected mesh, and the result passes a check that shares no code with
the twin."""
import os

import numpy as np
import pytest

import contiguity_ref as R
import reach_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", X.CASES)
def test_fix_is_the_contiguity_twins(name):
    d = X.case(name)
    fixed, st = R.fix(d["m"], d["mark0"].copy(), X.COLORS)
    assert np.array_equal(fixed, d["fixed"])
    assert st["counter"] == d["fix_counter"]
    f = d["fix_stats"]
    assert (st["nmerged"], st["nmerged_tets"], st["ncannot"]) == (f["fix_nmerged"], f["fix_nmerged_tets"],
                                                                 f["fix_ncannot"])


@pytest.mark.parametrize("name", X.CASES + ["interface6", "planted12", "cascade6", "unset_small_first"])
def test_flags_after_the_fix_are_a_function_of_the_marks(name):
    """flag != 0 <=> the mark is one of the colours the fix processed, and the
    fix's counter is the number of flagged tets."""
    if name in X.CASES:
        d = X.case(name)
        m, mark, colors = d["m"], d["mark0"], X.COLORS
    else:
        m, mark, col = R.case(name)[:3]
        colors = np.arange(col, dtype=np.int32) if np.ndim(col) == 0 else col
    t = X.Twin(m, mark)
    fixed, st = t.fix(colors)
    assert np.array_equal(t.flag[1:] != 0, np.isin(fixed, colors))
    assert st["counter"] == int(np.count_nonzero(t.flag[1:]))


@pytest.mark.parametrize("name", X.CASES)
def test_counter_and_flags_at_the_end(name):
    d = X.case(name)
    assert d["stats"]["counter"] == d["m"].ne and d["all_flagged"]
    s = d["stats"]
    assert s["nunreached"] == s["nmerged"] + s["ncannot"]
    # the tets whose mark changed were recoloured at least once
    assert int((d["mark"] != d["fixed"]).sum()) <= s["nmerged_tets"]
    # a local colour never changes, and no tet of a local colour is made
    assert np.array_equal(np.isin(d["fixed"], X.COLORS) & (d["mark"] != d["fixed"]), np.zeros(d["m"].ne, bool))


@pytest.mark.parametrize("name", X.CASES)
def test_result_against_numpy(name):
    d = X.case(name)
    assert X.numpy_check(d["m"], d["mark"], d["fi"], d["cin"]) == d["stats"]["ncannot"]


def test_the_cases_exercise_what_they_are_named_for():
    s = lambda n: X.case(n)["stats"]
    d = X.case("local4")
    assert d["fix_stats"]["fix_nmerged"] > 0 and s("local4")["nseeds"] == 0 and np.array_equal(d["mark"], d["fixed"])
    d = X.case("reached6")
    assert s("reached6")["nreached"] == 2 and s("reached6")["nunreached"] == 0 and np.array_equal(d["mark"], d["fixed"])
    for n in ("reached6@other", "reached6@unset"):
        assert s(n)["nreached"] == 0 and s(n)["nmerged"] == 2 and not np.isin(X.case(n)["mark"], [0, 2]).any()
    assert s("fragments6")["nmerged"] >= 6
    assert s("nested6")["nrescanned"] >= 1 and s("nested6")["nchained"] >= 1
    assert s("beside6")["nrescanned"] >= 1 and s("beside6")["nbeside_reached"] >= 1
    d = X.case("two_cubes@small_unset")
    assert d["stats"]["ncannot"] == 1 and np.all(d["mark"][:X.M.kuhn_cube(3).ne] == 3)
    d = X.case("fragments6@dup")
    assert len(np.unique(d["fi"])) < len(d["fi"]) and np.array_equal(d["mark"], X.case("fragments6")["mark"])
    assert any(s(n)["nrescanned"] > 10 for n in X.RANDOM_CASES)


def test_entry_out_of_range_is_refused():
    d = X.case("local4")
    t = X.Twin(d["m"], d["mark0"])
    t.fix()
    before = t.mark
    for bad in (0, 11, 12 * (d["m"].ne + 1)):
        ok, mark, _ = t.reach(np.array([bad], np.int32), np.array([1], np.int32))
        assert not ok and np.array_equal(mark, before)


def test_header_and_bindings_name_the_calls():
    from parmmg_amd import _native as N
    with open(os.path.join(ROOT, "include", "pmx_transfer.h"), encoding="utf-8") as fh:
        hdr = fh.read()
    for name in ("pmx_reach_face_marks", "pmx_check_reachability", "pmx_moveifc_fix", "pmx_moveifc_reach"):
        assert name + "(" in hdr and name in N.SIGNATURES
    assert "PMMG_check_reachability (src/moveinterfaces_pmmg.c:627-811) ->" in hdr
    assert [f for f, _ in N.ReachStats._fields_][:9] == list(X.REACH_FIELDS)
