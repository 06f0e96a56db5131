"""GPU: the located element, status, edge and vertex of every run mode against
the brute-force long-double definition of tests/reference_locate.py.

The other suites compare the location with the oracle only, a restatement
that shares the face-normal barycentrics, the closest rule, the hausd test and
the wedge / cone predicates with the kernels.  Here every input of
tests/locate_cases.py goes through the step in every run mode and then through
check_volume / check_surface: the element holds its point by determinant
ratios, nothing found is reported as not found and nothing found is missed,
the closest element is the closest, a tie on a jittered Kuhn mesh is answered
with the smallest index, and an edge / vertex answer satisfies its border,
wedge or cone predicate.  The long-double tables depend on mesh and points
only: computed once per input, shared by the modes.

Each run is also held to the oracle by the project's rules (compare_volume,
compare_exact from the recorded starts), so a disagreement says which side
left the definition; and on the ridge set and the L-shape, where wedge, cone
and closest-vertex values actually occur, a scalar and a generic tensor field
go through reference_hp.interp_errors (8 x the measured float64 floor).
"""
import numpy as np
import pytest

import locate_cases as LC
import reference_hp as R
import reference_locate as RL
from helpers import bits_equal, compare_exact, compare_volume, first_visit_order, generic_tensor
from oracle import oracle as O
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from test_gpu_pointmap import expected_starts

pytestmark = pytest.mark.gpu

REFWALK, NOTIES, FRESH, SERIAL = (N.RUN_REFERENCE_WALK, N.RUN_NO_INLINE_TIES, N.RUN_FRESH_BACKGROUND,
                                  N.RUN_SERIAL_SURFACE)
SEQ = N.RUN_SEQUENTIAL_SURFACE | N.RUN_SEQUENTIAL_VOLUME
SENT = R.SENT

# mode -> run options; "pointmap": sources uploaded, walks start from them
VOLUME_MODES = {"default": {}, "refwalk": dict(flags=REFWALK), "noties": dict(flags=NOTIES),
                "refwalk-noties": dict(flags=REFWALK | NOTIES), "fresh": dict(flags=FRESH),
                "maxwalk1": dict(max_walk=1), "pointmap": dict(pointmap=True)}
# (max_walk caps the volume walk only; the surface walks' overflow pass and
# exhaustive scan are reached by the far starts of the pointmap mode)
SURFACE_MODES = {"default": {}, "fresh": dict(flags=FRESH), "serial": dict(flags=SERIAL),
                 "maxwalk3": dict(max_walk=3), "pointmap": dict(pointmap=True)}
WITH_FIELDS = ("lshape", "ridge", "ridge_h002")      # inputs whose values also go through reference_hp


def fields(name, m):
    """[metric, scalar]: a generic tensor where the values are checked against
    the reference too (unit-cube meshes), the shock metric elsewhere; the
    scalar is positive everywhere (the errors are relative to the value)."""
    met = M.on_vertices(m, generic_tensor if name in WITH_FIELDS else M.shock_metric)
    return [met, M.on_vertices(m, M.iso_metric)]


def sources(m, x, t, seed=5):
    """A random old vertex per point (a boundary vertex for a surface point:
    the others start from tria 1 anyway), some 0 and some out of range."""
    rng = np.random.default_rng(seed)
    bv = np.unique(m.tria[1:].ravel())
    src = np.where((t & M.TAG_BDY) != 0, rng.choice(bv, len(x)), rng.integers(1, m.np + 1, len(x))).astype(np.int32)
    src[3::11] = 0
    src[7::29] = m.np + 3
    return src


def step(tr, m, x, t, sols, flags=0, max_walk=0, pointmap=False, tets_mmg=None):
    tr.upload_background(m, sols, 0)
    tr.upload_points(x, t, tets_mmg=tets_mmg)
    if pointmap:
        src = sources(m, x, t)
        tr.upload_point_sources(src)
    tr.run(flags=flags, max_walk=max_walk, pointmap=pointmap, record_starts=True)
    r = tr.download(init=[np.full((len(x), s.shape[1]), SENT) for s in sols])
    e, v = tr.border()
    starts = tr.starts()
    if pointmap:
        assert np.array_equal(starts, expected_starts(m, t, src))
    return r, starts, e, v


def oracle_from(m, x, t, sols, starts):
    """The oracle in the device's semantics from the device's starts."""
    o = O.Oracle(m)
    outs, elem, st, _, e, v = o.interp(x, t, sols, imet=0, fresh=True, start_vol=starts, start_bdy=starts,
                                       init=[np.full((len(x), s.shape[1]), SENT) for s in sols])
    return o, outs, elem, st, e, v


def check_values(name, mode, m, x, t, sols, r, e, v):
    """Metric and scalar against reference_hp at the device's own elements;
    the rows are reported (and bounded) per class of answer."""
    bdy = (t & M.TAG_BDY) != 0
    classes = {"found": r.status != 0, "closest": r.status == 0}
    if bdy.any():
        lam, _ = RL.tria_lambdas(m.xyz[m.tria[r.elem]], x)
        wedge = (e != -1) & (lam[np.arange(len(x)), np.maximum(e, 0)] <= -RL.EPS)
        classes = {"wedge": wedge, "vertex": v != -1, "other": ~wedge & (v == -1)}
    for k, s in enumerate(sols):
        floor, err, w = R.interp_errors(m, x, t, r.elem, r.status, s, r.sols[k], edge=e, vert=v, metric=k == 0)
        assert w.all()
        for cls, sel in classes.items():
            if sel.any():
                print(f"{name} {mode} size {s.shape[1]} {cls} ({int(sel.sum())}): floor {float(floor[sel].max()):.3g} "
                      f"device {float(err[sel].max()):.3g}")
                assert err[sel].max() <= 8 * floor[sel].max(), (name, mode, k, cls)


@pytest.mark.parametrize("mode", VOLUME_MODES)
@pytest.mark.parametrize("name", LC.VOLUME)
def test_volume(transfer, name, mode):
    m, x = LC.volume_case(name)
    ref = LC.volume_reference(name)
    t = np.zeros(len(x), np.uint16)
    sols = fields(name, m)
    r, starts, e, v = step(transfer, m, x, t, sols, **VOLUME_MODES[mode])
    canonical = name in LC.CUBES          # a tie across a > 10x size jump may stay uncanonical (wave)
    rep = RL.check_volume(m, x, r.elem, r.status, canonical, ref)
    print(name, mode, RL.summary(rep))
    assert not rep["violations"], rep["violations"][:5]
    assert rep["undecidable"] == 0
    rep["found"] += rep["exhaustive"]
    LC.assert_min_counts(rep, LC.VOLUME_MIN[name], (name, mode))
    if mode == "maxwalk1":
        assert rep["exhaustive"] >= 0.1 * rep["found"], "the capped walk must leave points to k_fallback"
    assert np.all(e == -1) and np.all(v == -1)
    o, outs, elem, st, _, _ = oracle_from(m, x, t, sols, starts)
    assert not RL.check_volume(m, x, elem, st, False, ref)["violations"]
    compare_volume(o, x, t, (r.sols, r.elem, r.status), (outs, elem, st), sols)
    if name in WITH_FIELDS:
        assert (r.status == 0).sum() >= 250
        check_values(name, mode, m, x, t, sols, r, e, v)


@pytest.mark.parametrize("mode", SURFACE_MODES)
@pytest.mark.parametrize("name", LC.SURFACE)
def test_surface(transfer, name, mode):
    m, x = LC.surface_case(name)
    ref = LC.surface_reference(name)
    t = np.full(len(x), M.TAG_BDY, np.uint16)
    sols = fields(name, m)
    r, starts, e, v = step(transfer, m, x, t, sols, **SURFACE_MODES[mode])
    rep = RL.check_surface(m, x, r.elem, r.status, e, v, ref)
    print(name, mode, RL.summary(rep))
    assert not rep["violations"], rep["violations"][:5]
    assert rep["undecidable"] == 0
    assert np.all(r.status[ref["nT"] > 0] != 0)
    o, outs, elem, st, eo, vo = oracle_from(m, x, t, sols, starts)
    repo = RL.check_surface(m, x, elem, st, eo, vo, ref)
    assert not repo["violations"], repo["violations"][:5]
    # the same counts on both sides; the flag-skip cone answers are the oracle's
    assert RL.summary(rep) == RL.summary(repo) and rep["skipped"] == repo["skipped"]
    if mode != "pointmap":
        # (a far start reaches a ridge point's edge from one side only: fewer wedge
        # and cone answers, more not found -- the definition holds either way)
        LC.assert_min_counts(rep, LC.SURFACE_MIN[name], (name, mode))
        assert not rep["skipped"]
    else:
        least = {"lshape6": 8, "wave": 100}.get(name, 0)
        assert rep["exhaustive"] >= least, "the far starts must reach the exhaustive scan"
    compare_exact((r.sols, r.elem, r.status, e, v), (outs, elem, st, eo, vo), np.arange(len(x)), len(sols))
    if name in WITH_FIELDS:
        check_values(name, mode, m, x, t, sols, r, e, v)


@pytest.mark.parametrize("mode", ["default", "pointmap"])
def test_cone_flag_skip(transfer, mode):
    """The input on which the oracle's walk from tria 1 accepts one cone
    through the reference's point-flag skip (locate_cases "wave_skip"):
    whichever answers the device's paths reach, they satisfy the definition,
    and the cone answers that fail the full predicate are exactly the
    oracle's from the same starts."""
    m, x = LC.surface_case("wave_skip")
    ref = LC.surface_reference("wave_skip")
    t = np.full(len(x), M.TAG_BDY, np.uint16)
    sols = fields("wave_skip", m)
    r, starts, e, v = step(transfer, m, x, t, sols, **SURFACE_MODES[mode])
    rep = RL.check_surface(m, x, r.elem, r.status, e, v, ref)
    print(mode, RL.summary(rep), rep["skipped"])
    assert not rep["violations"], rep["violations"][:5]
    assert rep["undecidable"] == 0 and len(rep["skipped"]) <= 2
    o, outs, elem, st, eo, vo = oracle_from(m, x, t, sols, starts)
    repo = RL.check_surface(m, x, elem, st, eo, vo, ref)
    assert RL.summary(rep) == RL.summary(repo) and rep["skipped"] == repo["skipped"]
    compare_exact((r.sols, r.elem, r.status, e, v), (outs, elem, st, eo, vo), np.arange(len(x)), len(sols))


def test_sequential(transfer):
    """The reference's sequential order (both paths): the walks start where
    the previous point ended and the point flags carry over, so the volume
    ties are the reference's (membership only); the surface answers satisfy
    the same predicates."""
    n = 6
    m = M.kuhn_cube(n)
    x, t = M.new_points(n)
    tets = M.new_point_tets(n, x, t)
    sols = fields("newpts6", m)
    r, _, e, v = step(transfer, m, x, t, sols, flags=SEQ, tets_mmg=tets)
    vol, bdy = t == 0, t != 0
    assert np.array_equal(x[vol], LC.volume_case("newpts6")[1])
    assert np.array_equal(x[bdy], LC.surface_case("newpts6")[1])
    rv = RL.check_volume(m, x[vol], r.elem[vol], r.status[vol], False, LC.volume_reference("newpts6"))
    rs = RL.check_surface(m, x[bdy], r.elem[bdy], r.status[bdy], e[bdy], v[bdy], LC.surface_reference("newpts6"))
    print(RL.summary(rv), RL.summary(rs))
    for rep in (rv, rs):
        assert not rep["violations"], rep["violations"][:5]
        assert rep["undecidable"] == 0
    assert rv["found"] == vol.sum() and rs["inside"] + rs["border_edge"] + rs["border_vertex"] == bdy.sum()
    assert not rs["skipped"]
    outs, elem, st, _, eo, vo = O.Oracle(m).interp(x, t, sols, imet=0, order=first_visit_order(tets, len(x)))
    compare_exact((r.sols, r.elem, r.status, e, v), (outs, elem, st, eo, vo), np.nonzero(bdy)[0], len(sols))
    assert np.array_equal(r.elem[vol], elem[vol]) and np.array_equal(r.status[vol], st[vol])
    for a, b in zip(r.sols, outs):
        assert bits_equal(a[vol], b[vol]).all()
