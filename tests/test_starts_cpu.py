"""CPU: the conditions the start tests rest on, and the definitions' teeth.

tests/test_gpu_starts.py holds the device's hint grids and starts to
tests/start_ref.py on the geometries of tests/geometry_cases.py, and the
located elements and values on the power-of-two images to the base run.  Here,
without a GPU:

* the oracle shows exactly those invariances, so a difference on the device is
  the device's (volume points on plate / rod / slab; everything, surface points
  included, under a uniform 2^-40 .. 2^30);
* the conditions hold from the definitions: both clamps are reached on the rod,
  the graded mesh leaves 320 of 512 cells empty with 86 of the 512 new points
  in one, at least 50 found points of it start through the shell search, a
  stride-64 grid leaves found points beyond three shells, no image is
  inverted, and the oracle's answers leave reference_locate nothing
  undecidable where its absolute TOL applies;
* every mutation a kernel could suffer is reported by start_ref's checks: a
  cell moved to its neighbour, a stale cell, a tria cell holding the second
  largest index, a shell scanned dx-first, radius 2 instead of 3.
"""
import dataclasses
import functools

import numpy as np
import pytest

import geometry_cases as G
import reference_locate as RL
import start_ref as S
from oracle import oracle as O
from parmmg_amd import mesh as M

SENT = -7.0


@functools.lru_cache(maxsize=None)
def oracle_run(name, scale=None):
    """The oracle alone (its own starts) on a geometry, or on the base
    geometry scaled uniformly by `scale` (hausd alike)."""
    m, x, t = G.case(name)
    if scale is not None:
        m = dataclasses.replace(m, xyz=m.xyz * scale, hausd=m.hausd * scale)
        x = x * scale
    sols = G.fields(m)
    outs, elem, st, steps, e, v = O.Oracle(m).interp(x, t, sols, imet=0, fresh=True,
                                                     init=[np.full((len(x), s.shape[1]), SENT) for s in sols])
    return G.Run(outs, elem, st, steps, e, v)


@functools.lru_cache(maxsize=None)
def nominal(name, stride=0, order=0):
    """(volume grid, tria grid) of a geometry by the definitions, each (desc, cells)."""
    m, _, _ = G.case(name)
    dv, dt = S.nominal_desc(m, 0), S.nominal_desc(m, 1)
    return (dv, S.some_volume_cells(m, dv, stride, order)), (dt, S.tria_cells(m, dt))


# ---- the oracle's invariances --------------------------------------------------------------

@pytest.mark.parametrize("name", G.ANISO)
def test_oracle_volume_invariance(name):
    _, _, t = G.case(name)
    G.assert_volume_invariant(name, t, oracle_run("base"), oracle_run(name))


@pytest.mark.parametrize("name", G.UNIFORM)
def test_oracle_uniform_invariance(name):
    _, _, t = G.case(name)
    G.assert_identical(name, np.arange(len(t)), oracle_run("base"), oracle_run(name))


@pytest.mark.parametrize("exp", (-40, 30))
def test_oracle_uniform_invariance_far(exp):
    """The surface points much further out.  (Not the volume points: the
    closest-tet search of a not-found point starts from an absolute 1e10,
    which a mesh of size 2^30 exceeds.)"""
    _, _, t = G.case("base")
    G.assert_identical(exp, np.nonzero(t != 0)[0], oracle_run("base"), oracle_run("base", 2.0 ** exp))


# ---- the conditions ------------------------------------------------------------------------

def test_points_and_meshes():
    _, x, t = G.case("base")
    assert (t == 0).sum() == 712 and (t != 0).sum() == 384
    for name in G.NAMES:
        m, xi, _ = G.case(name)
        assert m.ne == 3072 and m.nt == 768 and M.count_inverted(m) == 0, name
        assert np.isfinite(xi).all() and xi.shape == x.shape


def test_rod_reaches_both_clamps():
    m, _, _ = G.case("rod")
    lo, hi = S.bbox(m)
    ext = hi - lo
    hv = np.cbrt(ext.prod() / (m.ne / 6.0))
    ht = np.sqrt(2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) / (m.nt / 8.0))
    assert ext[0] / hv > 2 * S.VOL_CAP and ext[0] / ht > 1.1 * S.TRIA_CAP      # far from the cap: no rounding question
    assert ext[1] / hv < 1 and ext[2] / ht < 1
    (dv, _), (dt, _) = nominal("rod")
    assert list(dv["dim"]) == [4096, 1, 1] and list(dv["qf"]) == [9, 21, 21]
    assert list(dt["dim"]) == [1024, 1, 1]


def test_thin_grids_are_not_cubical():
    for name, flat in (("plate", 2), ("slab", 2)):
        (dv, _), (dt, _) = nominal(name)
        assert dv["dim"][flat] == 1 and dt["dim"][flat] == 1 and dv["dim"][0] > 8 * dv["dim"][flat]
    (dv, cells), _ = nominal("corner")
    assert list(dv["dim"]) == [8, 8, 8] and dv["lo"].min() >= 0.875


def test_graded_counts():
    m, x, t = G.case("graded")
    (dv, cells), tg = nominal("graded")
    assert cells.size == 512 and (cells == 0).sum() == 320
    _, radius = S.expected_starts(x, t, (dv, cells), tg)
    assert (radius[:896][t[:896] == 0] != 0).sum() == 86          # of the 512 new volume points
    found = (oracle_run("graded").status != 0) & (t == 0)
    assert (radius[found] > 0).sum() >= 50


@pytest.mark.parametrize("name", ("graded", "plate", "rod", "slab"))
def test_stride64_leaves_found_points_beyond_the_shells(name):
    m, x, t = G.case(name)
    (dv, cells), tg = nominal(name, 64)
    start, radius = S.expected_starts(x, t, (dv, cells), tg)
    far = (radius < 0) & (t == 0) & (oracle_run(name).status != 0)
    assert far.sum() >= 1 and np.all(start[far] == 1)


def test_definitions_hold_for_their_own_grids():
    for name in G.NAMES:
        m, x, t = G.case(name)
        for stride, order in ((0, 0), (1, 0), (64, 0), (0, 2)):
            (dv, cells), (dt, tc) = nominal(name, stride, order)
            assert not S.check_sizing(m, dv, cells.size, 0) and not S.check_sizing(m, dt, tc.size, 1)
            assert not S.check_volume_cells(m, dv, cells, stride, order), (name, stride, order)
            low = S.some_volume_cells(m, dv, stride, order, pick=min)         # any sampled tet of the cell is right
            assert not S.check_volume_cells(m, dv, low, stride, order)
            assert not S.check_tria_cells(m, dt, tc)


@pytest.mark.parametrize("name", G.REFERENCED)
def test_oracle_leaves_nothing_undecidable(name):
    m, x, t = G.case(name)
    rv, rs = G.references(name)
    r = oracle_run(name)
    vol, bdy = t == 0, t != 0
    rep = RL.check_volume(m, x[vol], r.elem[vol], r.status[vol], False, rv)
    reps = RL.check_surface(m, x[bdy], r.elem[bdy], r.status[bdy], r.edge[bdy], r.vertex[bdy], rs)
    for q in (rep, reps):
        assert not q["violations"], q["violations"][:5]
        assert q["undecidable"] == 0
    assert rep["found"] + rep["exhaustive"] >= 600 and rep["not_found"] >= 50
    assert not reps["skipped"] and reps["not_found"] == 0


# ---- the mutations ---------------------------------------------------------------------------

def test_sizing_mutations_are_reported():
    m, _, _ = G.case("slab")
    (dv, cells), (dt, tc) = nominal("slab")
    for key, a, val in (("lo", 0, np.nextafter(dv["lo"][0], 1.0)), ("inv", 1, np.nextafter(dv["inv"][1], 0.0)),
                        ("dim", 0, dv["dim"][0] + 2), ("qf", 0, dv["qf"][0] + 1)):
        d = {k: v.copy() for k, v in dv.items()}
        d[key][a] = val
        assert S.check_sizing(m, d, cells.size, 0), key
    # another mesh's box (an install path that takes its bounding box elsewhere)
    other, _, _ = G.case("base")
    assert S.check_sizing(m, S.nominal_desc(other, 0), 512, 0) and S.check_sizing(m, S.nominal_desc(other, 1), 64, 1)
    assert S.check_sizing(m, dv, cells.size + 1, 0)


@pytest.mark.parametrize("name", ("base", "graded", "slab"))
def test_volume_cell_mutations_are_reported(name):
    m, _, _ = G.case(name)
    (dv, cells), _ = nominal(name)
    flat = cells.ravel()
    nz = np.nonzero(flat)[0]
    # a cell moved to its neighbour (k_hint_build storing k + 1: the tet after a
    # sampled one is no sampled tet)
    g = flat.copy()
    g[nz] += 1
    assert S.check_volume_cells(m, dv, g)
    g = flat.copy()
    a = nz[len(nz) // 2]
    b = a + 1 if a + 1 < len(flat) else a - 1
    g[b], g[a] = g[a], 0
    assert S.check_volume_cells(m, dv, g)
    # a stale cell: an empty cell keeps a tet (here a sampled one, of another cell)
    g = flat.copy()
    empty = np.nonzero(flat == 0)[0]
    if len(empty):
        g[empty[0]] = flat[nz[0]]
        assert S.check_volume_cells(m, dv, g)
    # ... or a grid left as another stride built it
    (_, other) = nominal(name, 1)[0]
    assert S.check_volume_cells(m, dv, other, 64)
    # an empty grid
    assert S.check_volume_cells(m, dv, np.zeros_like(flat))
    # a tet past ne
    g = flat.copy()
    g[nz[0]] = m.ne + 1
    assert S.check_volume_cells(m, dv, g)


@pytest.mark.parametrize("name", ("base", "rod", "graded"))
def test_tria_cell_mutations_are_reported(name):
    m, _, _ = G.case(name)
    _, (dt, tc) = nominal(name)
    # the second largest index of a cell (atomicMin instead of atomicMax gives the smallest)
    ks = np.arange(1, m.nt + 1)
    P = m.xyz[m.tria[ks]]
    c = S._cell_coords(((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0, dt)
    cell = c[:, 0] + dt["dim"][0] * (c[:, 1] + dt["dim"][1] * c[:, 2])
    ids, cnt = np.unique(cell, return_counts=True)
    multi = ids[cnt > 1]
    assert len(multi), "no cell holds two trias"
    second = np.sort(ks[cell == multi[0]])[-2]
    g = tc.ravel().copy()
    g[multi[0]] = second
    assert S.check_tria_cells(m, dt, g)
    low = np.zeros_like(g)
    low[cell[::-1]] = ks[::-1]                   # the smallest per cell
    assert S.check_tria_cells(m, dt, low)


def test_start_mutations_are_reported():
    """On the graded mesh the shell order and the radius both decide starts."""
    m, x, t = G.case("graded")
    (dv, cells), (dt, tc) = nominal("graded", 64)
    vol = t == 0
    want, radius = S.hint_starts(dv, cells, x[vol], S.VOL_SHELLS)
    assert (radius > 0).sum() >= 50 and (radius == 3).sum() >= 1 and (radius < 0).sum() >= 1
    starts = np.zeros(len(x), np.int64)
    starts[~vol], _ = S.hint_starts(dt, tc, x[~vol], S.TRIA_SHELLS)
    for kw in (dict(shells=S.VOL_SHELLS, order="xyz"), dict(shells=2), dict(shells=4)):
        starts[vol], _ = S.hint_starts(dv, cells, x[vol], **kw)
        assert S.check_starts(x, t, starts, (dv, cells), (dt, tc)), kw
    starts[vol] = want
    assert not S.check_starts(x, t, starts, (dv, cells), (dt, tc))
    # the surface search likewise (the rod's tria grid has empty cells beyond 4 shells)
    m, x, t = G.case("rod")
    (dv, cells), (dt, tc) = nominal("rod")
    vol = t == 0
    starts = np.zeros(len(x), np.int64)
    starts[vol], _ = S.hint_starts(dv, cells, x[vol], S.VOL_SHELLS)
    _, rb = S.hint_starts(dt, tc, x[~vol], S.TRIA_SHELLS)
    assert (rb == 4).sum() >= 1 and (rb < 0).sum() >= 1
    for kw in (dict(shells=3), dict(shells=5)):
        starts[~vol], _ = S.hint_starts(dt, tc, x[~vol], **kw)
        assert S.check_starts(x, t, starts, (dv, cells), (dt, tc)), kw
    # a start that ignores the grid
    starts[~vol] = 1
    assert S.check_starts(x, t, starts, (dv, cells), (dt, tc))
