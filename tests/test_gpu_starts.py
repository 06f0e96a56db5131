"""GPU: where the walks start, and the geometry the starts are built from.

Every parity test replays the oracle from the device's own starts, so nothing
said what a start has to be.  Here the hint grids a step built
(Transfer.debug_grid) and the starts it recorded are held to the definitions of
tests/start_ref.py -- sizing, volume cells, tria cells, shell search, all by
equality -- on the geometries of tests/geometry_cases.py: a plate, a rod that
reaches both grid clamps, a slab, the same mesh 2^-20 and 2^12 times its size,
a sub-box away from the origin and a graded mesh that leaves most cells empty.

Run modes: default, FRESH, REFWALK, hint_stride 1 and 64, and (in a child
process: the switch is read at the upload) PMX_HINT_SAMPLE_ORDER=2.  Every one
of them records the start the rule gives.  The modes that record something
else are not run here and are pinned elsewhere: a PMX_RUN_POINTMAP step builds
no grid and starts from the sources' first incident elements
(test_gpu_pointmap.expected_starts), a PMX_RUN_SEQUENTIAL_* step starts each
query where the previous one ended (test_gpu_seq_surface).

Each step is also held to the oracle from its starts (compare_volume,
compare_exact) and, where reference_locate's absolute TOL applies, to the
long-double definition.  The power-of-two images must reproduce the base run:
the volume points' elements and found values on plate / rod / slab, everything
on tiny / huge.  One equality cannot be had between two runs: k_hint_build
fills a cell with a plain store, so where a cell holds more than one sampled
tet two runs may start a volume walk at different tets (test_gpu_pointmap.
test_default_unchanged measured 2-3 of 512).  The start itself is pinned above
run by run; between the base and the tiny / huge run, steps and the sign of a
found status are compared where the two starts are equal, a differing pair of
starts must both be sampled tets of the same cell, and everything else --
elem, found or not, edge, vertex, every field -- is compared for every point.

Which assertion a planted kernel bug fails: k_hint_build storing k + 1, or a
grid that is not cleared (stale cells of the previous background or stride),
fails check_volume_cells in test_cells_and_starts / test_no_stale_cells;
atomicMin in tria_hint_one fails check_tria_cells; hint_search with its loops
swapped, or another radius, fails check_starts on `graded` (where at least 50
found points start through the shells) and with stride 64; an install path
with another bounding box fails check_sizing in test_install_paths.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_cases as G
import reference_locate as RL
import start_ref as S
from conftest import ROOT
from helpers import compare_exact, compare_volume
from oracle import oracle as O
from parmmg_amd import _native as N
from parmmg_amd import mesh as M

pytestmark = pytest.mark.gpu

SENT = -7.0
MODES = {"default": {}, "fresh": dict(flags=N.RUN_FRESH_BACKGROUND), "refwalk": dict(flags=N.RUN_REFERENCE_WALK),
         "stride1": dict(hint_stride=1), "stride64": dict(hint_stride=64)}
_runs = {}


def step(tr, m, x, t, sols, upload=True, **opts):
    """One recorded step: (Run, starts, volume grid, tria grid)."""
    if upload:
        tr.upload_background(m, sols, 0)
    tr.upload_points(x, t)
    tr.run(record_starts=True, **opts)
    r = tr.download(init=[np.full((len(x), s.shape[1]), SENT) for s in sols])
    e, v = tr.border()
    tg = tr.debug_grid(1) if ((t & M.TAG_BDY) != 0).any() else None
    return G.Run(r.sols, r.elem, r.status, r.steps, e, v), tr.starts(), tr.debug_grid(0), tg


def run_of(tr, name, mode):
    """The step of a geometry in a mode, run once per session."""
    if (name, mode) not in _runs:
        m, x, t = G.case(name)
        _runs[name, mode] = step(tr, m, x, t, G.fields(m), **MODES[mode])
    return _runs[name, mode]


def check_grids(m, x, t, starts, vg, tg, stride=0, order=0):
    """Sizing, cells and starts against start_ref; returns the radius per point."""
    bad = S.check_sizing(m, vg[0], vg[1].size, 0) + S.check_volume_cells(m, vg[0], vg[1], stride, order)
    if tg is not None:
        bad += S.check_sizing(m, tg[0], tg[1].size, 1) + S.check_tria_cells(m, tg[0], tg[1])
    bad += S.check_starts(x, t, starts, vg, tg)
    assert not bad, bad
    return S.expected_starts(x, t, vg, tg)[1]


def check_located(m, x, t, sols, r, starts, refs=None):
    """The step against the oracle from its starts and, with refs, against
    the long-double definition."""
    o = O.Oracle(m)
    outs, elem, st, _, eo, vo = o.interp(x, t, sols, imet=0, fresh=True, start_vol=starts, start_bdy=starts,
                                         init=[np.full((len(x), s.shape[1]), SENT) for s in sols])
    compare_volume(o, x, t, (r.sols, r.elem, r.status), (outs, elem, st), sols)
    bdy = np.nonzero((t & M.TAG_BDY) != 0)[0]
    if len(bdy):
        compare_exact((r.sols, r.elem, r.status, r.edge, r.vertex), (outs, elem, st, eo, vo), bdy, len(sols))
    if refs is None:
        return
    vol, bdy = t == 0, t != 0
    rv = RL.check_volume(m, x[vol], r.elem[vol], r.status[vol], False, refs[0])
    rs = RL.check_surface(m, x[bdy], r.elem[bdy], r.status[bdy], r.edge[bdy], r.vertex[bdy], refs[1])
    print(RL.summary(rv), RL.summary(rs))
    for rep in (rv, rs):
        assert not rep["violations"], rep["violations"][:5]
        assert rep["undecidable"] == 0
    assert rv["found"] + rv["exhaustive"] >= 600 and rv["not_found"] >= 50
    assert rs["not_found"] == 0 and not rs["skipped"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.NAMES)
def test_cells_and_starts(transfer, name, mode):
    m, x, t = G.case(name)
    r, starts, vg, tg = run_of(transfer, name, mode)
    radius = check_grids(m, x, t, starts, vg, tg, stride=MODES[mode].get("hint_stride", 0))
    found = (r.status != 0) & (t == 0)
    print(name, mode, "dims", vg[0]["dim"], tg[0]["dim"], "empty cells", int((vg[1] == 0).sum()), "of", vg[1].size,
          "found volume points by shell", int((radius[found] > 0).sum()), "beyond", int((radius[found] < 0).sum()))
    if name == "rod":
        assert list(vg[0]["dim"]) == [4096, 1, 1] and list(vg[0]["qf"]) == [9, 21, 21]
        assert list(tg[0]["dim"]) == [1024, 1, 1]
    if name == "graded" and mode != "stride1":
        assert (radius[found] > 0).sum() >= 50, "the shell search must decide starts"
    if name == "graded" and mode in ("default", "fresh", "refwalk"):
        assert (vg[1] == 0).sum() == 320


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.NAMES)
def test_located(transfer, name, mode):
    """The oracle from the step's starts, and reference_locate where its TOL
    applies (rod, tiny and huge rest on test_invariance, whose base case the
    reference pins here)."""
    m, x, t = G.case(name)
    r, starts, _, _ = run_of(transfer, name, mode)
    check_located(m, x, t, G.fields(m), r, starts, G.references(name) if name in G.REFERENCED else None)


@pytest.mark.parametrize("name", ("graded", "plate", "rod", "slab"))
def test_stride64_beyond_three_shells(transfer, name):
    """A found point with no sampled tet within three shells starts at tet 1
    and is still located where the default run locates it."""
    m, x, t = G.case(name)
    r, starts, vg, tg = run_of(transfer, name, "stride64")
    radius = S.expected_starts(x, t, vg, tg)[1]
    far = (radius < 0) & (t == 0) & (r.status != 0)
    assert far.sum() >= 1 and np.all(starts[far] == 1)
    d = run_of(transfer, name, "default")[0]
    assert np.array_equal(r.elem[far], d.elem[far]) and np.all(d.status[far] != 0)
    vol = t == 0
    assert np.array_equal(r.elem[vol], d.elem[vol]) and np.array_equal(r.status[vol] != 0, d.status[vol] != 0)


@pytest.mark.parametrize("name", G.ANISO + G.UNIFORM)
def test_invariance(transfer, name):
    m, x, t = G.case(name)
    b, sb, vgb, tgb = run_of(transfer, "base", "default")
    r, sr, vgr, tgr = run_of(transfer, name, "default")
    if name in G.ANISO:
        G.assert_volume_invariant(name, t, b, r)
        return
    # the precondition: the same grids
    for a, c in ((vgb, vgr), (tgb, tgr)):
        assert np.array_equal(a[0]["dim"], c[0]["dim"]) and np.array_equal(a[0]["qf"], c[0]["qf"])
    assert np.array_equal(tgb[1], tgr[1])
    bdy = np.nonzero(t != 0)[0]
    assert np.array_equal(sb[bdy], sr[bdy])
    G.assert_identical(name, bdy, b, r)
    vol = np.nonzero(t == 0)[0]
    same = sb[vol] == sr[vol]
    print(name, "volume starts that differ between the two runs:", int((~same).sum()), "of", len(vol))
    G.assert_identical(name, vol[same], b, r)
    G.assert_identical(name, vol[~same], b, r, walk=False)
    # a differing pair: both sampled tets of one cell (the racy store), nothing else
    mb, _, _ = G.case("base")
    ks = np.concatenate([sb[vol][~same], sr[vol][~same]])
    assert np.isin(ks, S.sample(mb)).all()
    assert np.array_equal(S.cell_of(mb, vgb[0], sb[vol][~same]), S.cell_of(m, vgr[0], sr[vol][~same]))
    assert same.mean() > 0.5


def test_no_stale_cells(transfer):
    """One context: a larger background first, then the 3072-tet mesh at
    stride 1 and at stride 64 -- non-zero iff a sampled tet, nothing past ne."""
    big = M.kuhn_cube(12)
    xb, tb = M.new_points(12)
    sb = [M.on_vertices(big, M.shock_metric), M.on_vertices(big, M.iso_metric), M.on_vertices(big, M.velocity)]
    _, starts, vg, tg = step(transfer, big, xb, tb, sb)
    check_grids(big, xb, tb, starts, vg, tg)
    assert vg[1].size > 512
    for name in ("base", "graded"):
        m, x, t = G.case(name)
        sols = G.fields(m)
        upload = True
        for stride in (1, 64, 0):
            _, starts, vg, tg = step(transfer, m, x, t, sols, upload=upload, hint_stride=stride)
            upload = False                       # the next stride on the same background and points
            check_grids(m, x, t, starts, vg, tg, stride=stride)
            assert vg[1].max() <= m.ne and tg[1].max() <= m.nt
            if stride == 64:
                assert (vg[1] != 0).sum() <= 48


@pytest.mark.parametrize("name", ("corner", "slab"))
def test_install_paths(transfer, name):
    """pmx_promote_background, split_adopt and merge_adopt of the same mesh:
    the descriptors of a plain upload (the bounding box comes from the new
    points' or from the device there), cells and starts by the definitions."""
    import merge_ref as MR
    import split_ref as SP
    from parmmg_amd.transfer import Transfer
    m, x, t = G.case(name)
    sols = G.fields(m)
    _, _, vg0, tg0 = run_of(transfer, name, "default")

    def same_desc(a, b):
        for k in ("dim", "qf"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("lo", "inv"):
            assert a[k].tobytes() == b[k].tobytes(), k

    other = Transfer(0)
    try:
        # promotion: the mesh's own vertices as the new points, its tets as the new tets
        tets0 = (m.tet - 1).astype(np.int32)
        other.upload_background(m, sols, 0)
        other.upload_points(np.ascontiguousarray(m.xyz[1:]), np.zeros(m.np, np.uint16), tets=tets0)
        other.run()
        r = other.download(init=[np.ascontiguousarray(s[1:]) for s in sols])
        other.promote_background(m, r.sols)
        _, starts, vg, tg = step(other, m, x, t, sols, upload=False)
        same_desc(vg[0], vg0[0])
        same_desc(tg[0], tg0[0])
        check_grids(m, x, t, starts, vg, tg)
        # split_adopt of the one group that is the whole mesh
        transfer.upload_background(m, sols, 0)
        transfer.split_groups(np.zeros(m.ne, np.int32), 1)
        grp = transfer.split_fetch(0)
        mg = SP.group_mesh(grp)
        mg.hausd = m.hausd
        assert mg.ne == m.ne and mg.np == m.np
        transfer.split_adopt(0, other, imet=0, surface=True, hausd=m.hausd)
        transfer.split_release()
        _, starts, vg, tg = step(other, mg, x, t, grp["sols"], upload=False)
        _, _, vgu, tgu = step(transfer, mg, x, t, grp["sols"])
        same_desc(vg[0], vgu[0])
        same_desc(tg[0], tgu[0])
        same_desc(vg[0], vg0[0])
        check_grids(mg, x, t, starts, vg, tg)
        # merge_adopt of the mesh's two halves (no surface: volume points only)
        sp, comm = MR.split_case(m, SP.slabs(G.case("base")[0], 2), 2, sols)     # the same tets on every image
        other.merge_groups(sp["groups"], comm)
        d = other.merge_fetch()
        mm = M.from_tets(d["xyz"], d["tetra_v"], hausd=m.hausd)
        assert mm.ne == m.ne and mm.np == m.np
        other.merge_adopt(imet=0)
        other.merge_release()
        vol = t == 0
        xv, tv = np.ascontiguousarray(x[vol]), np.ascontiguousarray(t[vol])
        rr, starts, vg, tg = step(other, mm, xv, tv, d["sols"], upload=False)
        same_desc(vg[0], vg0[0])
        check_grids(mm, xv, tv, starts, vg, None)
        with pytest.raises(RuntimeError, match="no tria hint grid"):
            other.debug_grid(1)
        check_located(mm, xv, tv, d["sols"], rr, starts)
    finally:
        other.close()


def test_debug_grid_refusals(transfer):
    m, x, t = G.case("base")
    sols = G.fields(m)
    transfer.upload_background(m, sols, 0)
    with pytest.raises(RuntimeError, match="no step"):
        transfer.debug_grid(0)
    transfer.upload_points(x, t)
    transfer.upload_point_sources(np.ones(len(x), np.int32))
    transfer.run(pointmap=True)
    for which in (0, 1):
        with pytest.raises(RuntimeError, match="built no"):
            transfer.debug_grid(which)
    with pytest.raises(RuntimeError, match="which"):
        transfer.debug_grid(2)
    transfer.run()
    n = transfer.lib.pmx_debug_grid(transfer.ctx, 0, None, None, 0)
    assert n == 512
    short = np.full(n, -5, np.int32)
    assert transfer.lib.pmx_debug_grid(transfer.ctx, 0, None, short.ctypes.data_as(N.iptr), n - 1) == 0
    assert np.all(short == -5) and b"cap" in transfer.lib.pmx_last_error(transfer.ctx)
    old = np.zeros(n, np.int32)
    assert transfer.lib.pmx_debug_hint_grid(transfer.ctx, old.ctypes.data, n) == n
    assert np.array_equal(old, transfer.debug_grid(0)[1].ravel())


def _child():
    """PMX_HINT_SAMPLE_ORDER=2 (set by the parent): the vertex-owner sample at
    the default stride, the strided sample at stride 64, on every geometry."""
    from parmmg_amd.transfer import Transfer
    tr = Transfer(0)
    for name in G.NAMES:
        m, x, t = G.case(name)
        sols = G.fields(m)
        for stride in (0, 64):
            r, starts, vg, tg = step(tr, m, x, t, sols, hint_stride=stride)
            check_grids(m, x, t, starts, vg, tg, stride=stride, order=2)
            check_located(m, x, t, sols, r, starts)
            if stride == 0:
                assert np.isin(vg[1][vg[1] != 0], S.sample(m, 0, 2)).all()
        print(name, "owner sample: cells and starts by definition")
    tr.close()
    print("sample order 2 ok")


def test_sample_order_2():
    env = dict(os.environ, PMX_HINT_SAMPLE_ORDER="2")
    code = (f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); sys.path.insert(0, {ROOT!r}); "
            f"import test_gpu_starts as t; t._child()")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "sample order 2 ok" in r.stdout
