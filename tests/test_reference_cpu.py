"""The oracle's tensor formulas against an independent long-double reference.

tests/reference_hp.py states interpolation, quality and classic-storage edge
length from their definitions (3x3 matrices, long double).  Here the oracle --
the checker of every GPU test -- is compared with it on a generic tensor field
(helpers.generic_tensor: no two diagonal and no two off-diagonal entries
equal, so an index or storage-order mistake moves the result) on a Kuhn cube
and on the unstructured wave.0.mesh.

Tolerance: measured, not chosen.  For each quantity the noise floor is the
largest deviation between the reference evaluated in float64 and in long
double on the test's own inputs; the oracle must sit within 8 x that floor (a
different but equally valid float64 operation order over three chained
operations).  Counts and histograms are exact, after asserting that no
reference value lies within 1e-9 of a bin bound or threshold.
"""
import os

import numpy as np
import pytest

import reference_hp as R
from conftest import REF_INPUTS
from helpers import (generic_tensor, generic_tensor_edges, graded_iso_scaled, ridge_tags, unit_box)
from oracle import oracle as O
from parmmg_amd import mesh as M

LD = np.longdouble
SENT = R.SENT
SWAPS = [(i, j) for i in range(6) for j in range(i + 1, 6)]     # the 15 column pairs


def positive_vector(m):
    return np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), 2.0 + np.cos(2.0 * m.xyz[1:])]))


def wave_points(m, seed=4):
    """Points of an unstructured mesh: inside every 10th tet and on every 5th
    boundary tria, random barycentrics bounded away from the border; and the
    elements they were built in (the walks' starts: found at the first step,
    no surface point ends on a neighbour's edge or vertex)."""
    rng = np.random.default_rng(seed)
    tk, fk = np.arange(1, m.ne + 1, 10), np.arange(1, m.nt + 1, 5)
    wt = 0.05 + 0.8 * rng.dirichlet(np.ones(4), len(tk))
    wf = 0.1 + 0.7 * rng.dirichlet(np.ones(3), len(fk))
    x = np.concatenate([np.einsum("nk,nkd->nd", wt, m.xyz[m.tet[tk]]),
                        np.einsum("nk,nkd->nd", wf, m.xyz[m.tria[fk]])])
    t = np.concatenate([np.zeros(len(tk), np.uint16), np.full(len(fk), M.TAG_BDY, np.uint16)])
    return x, t, np.concatenate([tk, fk]).astype(np.int32)


@pytest.fixture(scope="module", params=["cube6", "wave"])
def case(request):
    if request.param == "cube6":
        m = M.kuhn_cube(6)
        x, t = M.new_points(6)
        start = None
        met = M.on_vertices(m, generic_tensor)
        iso = M.on_vertices(m, M.graded_iso_metric(6))
    else:
        m = M.read_medit(os.path.join(REF_INPUTS, "wave.0.mesh"))
        x, t, start = wave_points(m)
        met = M.on_vertices(m, unit_box(generic_tensor))
        iso = graded_iso_scaled(m)
    return request.param, m, x, t, met, iso, start


def test_generic_tensor_is_generic():
    """Every vertex of the meshes the tests use: the three diagonal entries
    pairwise different by more than 1e-3 relative, and the three off-diagonal
    entries too; symmetric positive definite."""
    wave = M.read_medit(os.path.join(REF_INPUTS, "wave.0.mesh"))
    for m, f in ((M.kuhn_cube(5), generic_tensor), (M.kuhn_cube(6), generic_tensor),
                 (M.kuhn_cube(7), generic_tensor), (wave, unit_box(generic_tensor))):
        met = M.on_vertices(m, f)[1:]
        for cols in ((0, 3, 5), (1, 2, 4)):
            a = np.abs(met[:, cols])
            for i, j in ((0, 1), (0, 2), (1, 2)):
                sep = np.abs(met[:, cols[i]] - met[:, cols[j]]) / np.maximum(a[:, i], a[:, j])
                assert sep.min() > 1e-3, (cols[i], cols[j], sep.min())
        ev = np.linalg.eigvalsh(R.full(met, np.float64))
        assert ev.min() > 0 and (ev[:, 2] / ev[:, 0]).max() < 200


def test_interpolation(case):
    """Volume and surface points, at the oracle's own located element: tensor,
    scalar and vector rows."""
    name, m, x, t, met, iso, start = case
    sols = [met, iso, positive_vector(m)]
    o = O.Oracle(m)
    outs, elem, st, _, e, v = o.interp(x, t, sols, imet=0, init=[np.full((len(x), s.shape[1]), SENT) for s in sols],
                                       fresh=start is not None, start_vol=start, start_bdy=start)
    assert np.all(st != 0) and np.all(e == -1) and np.all(v == -1)      # plain hits only
    bdy = (t & M.TAG_BDY) != 0
    assert bdy.sum() >= 100 and (~bdy).sum() >= 200
    for k, s in enumerate(sols):
        floor, err, w = R.interp_errors(m, x, t, elem, st, s, outs[k])
        assert w.all()
        for cls, sel in (("volume", ~bdy), ("surface", bdy)):
            print(f"{name} size {s.shape[1]} {cls}: floor {float(floor[sel].max()):.3g} "
                  f"oracle {float(err[sel].max()):.3g}")
            assert err[sel].max() <= 8 * floor[sel].max()


def test_planted_rows():
    """generic_tensor_edges on cube 6: rows on either side of the diagonal
    branch of the inversion follow the documented rule, and a point whose
    element holds the singular vertex keeps its init value."""
    m = M.kuhn_cube(6)
    x, t = M.new_points(6, surface=False)
    met, planted = generic_tensor_edges(m, M.on_vertices(m, generic_tensor))
    for name in ("zero", "below", "above"):
        offmax = np.abs(met[planted[name]][:, [1, 2, 4]]).max(axis=1)
        assert np.all(offmax == {"zero": 0.0, "below": 0.5e-6, "above": 2e-6}[name])
    allp = sum(planted.values(), [])
    tv = m.tet[1:]
    assert np.isin(tv, allp).sum(axis=1).max() == 1, "planted vertices must share no tet"
    o = O.Oracle(m)
    outs, elem, st, *_ = o.interp(x, t, [met], imet=0, init=[np.full((len(x), 6), SENT)])
    floor, err, w = R.interp_errors(m, x, t, elem, st, met, outs[0])
    sing = np.isin(m.tet[elem], planted["singular"]).any(axis=1)
    assert np.array_equal(~w, sing)
    assert 1 <= sing.sum() <= 0.05 * len(x)
    assert err.max() <= 8 * floor.max()
    # teeth: without the rule the rows planted below the threshold give another result
    plain, _ = R.interp_at(m, x, t, elem, st, met, LD, diag_rule=False)
    ref, _ = R.interp_at(m, x, t, elem, st, met, LD)
    below = np.isin(m.tet[elem], planted["below"]).any(axis=1) & w
    above = np.isin(m.tet[elem], planted["above"]).any(axis=1) & w
    zero = np.isin(m.tet[elem], planted["zero"]).any(axis=1) & w
    assert below.sum() >= 1 and above.sum() >= 1 and zero.sum() >= 1
    assert R.rel_rows(plain[below], ref[below]).min() > 1e3 * 8 * floor.max()
    other = w & ~below
    assert R.rel_rows(plain[other], ref[other]).max() <= 8 * floor.max()


def test_quality(case):
    name, m, x, t, met, iso, start = case
    T = m.tet[1:]
    P = m.xyz[T]
    for label, mm in (("iso", None), ("ani", met)):
        q = O.tetra_qual(m, mm)
        ref, floor, err = R.quality_errors(P, None if mm is None else mm[T], q[1:])
        print(f"{name} quality {label}: floor {float(floor.max()):.3g} oracle {float(err.max()):.3g}")
        assert err.max() <= 8 * floor.max()
        R.check_qual_stats(O.qualhisto(m, q), ref, T, None, 8 * float(floor.max()))


def test_quality_ridge():
    """The mean metric without the non-singular ridge points (cube 7, tags)."""
    m = M.kuhn_cube(7)
    tags = ridge_tags(m)
    met = M.on_vertices(m, generic_tensor)
    T = m.tet[1:]
    q = O.tetra_qual(m, met, tags=tags, met_rid_typ=1)
    ridge = R.is_ridge(tags)[T]
    assert ridge.all(axis=1).sum() > 0 and (ridge.any(axis=1) & ~ridge.all(axis=1)).sum() > 0
    ref, floor, err = R.quality_errors(m.xyz[T], met[T], q[1:], ridge)
    print(f"cube7 quality ridge: floor {float(floor.max()):.3g} oracle {float(err.max()):.3g}")
    assert err.max() <= 8 * floor.max()
    h = O.qualhisto(m, q, tags=tags)
    assert h["nrid"] > 0
    R.check_qual_stats(h, ref, T, tags, 8 * float(floor.max()))


def test_lengths(case):
    name, m, x, t, met, iso, start = case
    for label, mm in (("iso", iso), ("ani", met)):
        ed, ref, floor = R.length_reference(m, mm)
        s = R.check_len_stats(O.prilen(m, mm), ed, ref, 8 * floor)
        print(f"{name} length {label}: floor {floor:.3g} bins {s['hl']}")
        assert sum(1 for h in s["hl"] if h) >= (9 if name == "wave" else 5)


def test_lengths_ridge():
    m = M.kuhn_cube(7)
    tags = ridge_tags(m)
    met = M.on_vertices(m, generic_tensor)
    ed, ref, floor = R.length_reference(m, met, tags)
    assert len(ed) < len(R.unique_edges(m.tet[1:])), "the filter must bite"
    R.check_len_stats(O.prilen(m, met, tags=tags), ed, ref, 8 * floor)


def test_mutations(case):
    """Teeth: the metric with any two of its 6 columns swapped moves the
    reference by more than 1e6 x the tolerance on at least 90 % of the points,
    tets and edges -- a kernel that reads the wrong component cannot pass.
    (Lengths on the unstructured mesh only: a Kuhn cube's 13 % of edges in the
    faces x = 0 / 1 have a zero x component, which m11 and m12 both multiply.)"""
    name, m, x, t, met, iso, start = case
    o = O.Oracle(m)
    _, elem, st, *_ = o.interp(x, t, [met], imet=0, fresh=start is not None, start_vol=start, start_bdy=start)
    T = m.tet[1:]
    ed = R.unique_edges(T)

    def evaluate(mm, dtype=LD):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            a, _ = R.interp_at(m, x, t, elem, st, mm, dtype)
            return a, R.qual_ani(m.xyz[T], mm[T], dtype), R.len_ani33(m.xyz, mm, ed, dtype)
    base, b64 = evaluate(met), evaluate(met, np.float64)
    tol = (8 * float(R.rel_rows(b64[0], base[0]).max()), 8 * float((np.abs(b64[1] - base[1]) / base[1]).max()),
           8 * float((np.abs(b64[2] - base[2]) / base[2]).max()))
    for i, j in SWAPS:
        mm = met.copy()
        mm[:, [i, j]] = mm[:, [j, i]]
        mut = evaluate(mm)
        with np.errstate(invalid="ignore"):
            dev = (R.rel_rows(mut[0], base[0]), np.abs(mut[1] - base[1]) / base[1],
                   np.abs(mut[2] - base[2]) / base[2])
        for what, d, tl in zip(("interpolation", "quality", "length"), dev, tol):
            if what == "length" and name != "wave":
                continue
            moved = ~(d <= 1e6 * tl)                       # a NaN (no longer SPD) has moved
            assert moved.mean() >= 0.9, (what, i, j, moved.mean())
