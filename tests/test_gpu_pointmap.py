"""GPU: point-map starts (PMX_RUN_POINTMAP, the reference's USE_POINTMAP build).

Every walk starts from its point's source vertex: a surface point from the
smallest tria holding the vertex, a volume point from the smallest valid tet
holding it (PMMG_locate_setStart, src/locate_pmmg.c:931-986, whose loops keep
the first index that reaches a vertex), element 1 when the source is outside
1..np or no element holds it.  The expected starts are a numpy restatement of
those two minima; fed to the oracle as per-point starts they give the
reference answer the device must reproduce (surface: bit for bit; volume: the
same tet except documented ties, the cap of test_volume_parity).
"""
import numpy as np
import pytest

from helpers import bits_equal, compare_exact, compare_volume, cube_case, lin_field
from oracle import oracle as O
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

FRESH = N.RUN_FRESH_BACKGROUND
REFWALK = N.RUN_REFERENCE_WALK
BIG = np.iinfo(np.int64).max


def first_incident(m):
    """(vol_start, tri_start), np + 1 entries each: the smallest valid tet /
    the smallest tria holding each vertex, 0 if none."""
    vol = np.full(m.np + 1, BIG)
    tet = m.tet[1:]
    k = np.repeat(np.arange(1, m.ne + 1), 4).reshape(-1, 4)
    ok = tet[:, 0] > 0
    np.minimum.at(vol, tet[ok].ravel(), k[ok].ravel())
    tri = np.full(m.np + 1, BIG)
    if m.nt > 0:
        np.minimum.at(tri, m.tria[1:].ravel(), np.repeat(np.arange(1, m.nt + 1), 3))
    vol[vol == BIG] = 0
    tri[tri == BIG] = 0
    vol[0] = tri[0] = 0
    return vol, tri


def expected_starts(m, t, src):
    """The start element of every point from its source (1-based vertex)."""
    vol, tri = first_incident(m)
    s = np.asarray(src, np.int64)
    ok = (s >= 1) & (s <= m.np)
    sc = np.where(ok, s, 0)
    e = np.where((np.asarray(t) & M.TAG_BDY) != 0, tri[sc], vol[sc])
    return np.where(ok & (e > 0), e, 1).astype(np.int32)


def nearest_vertex(m, x, among=None):
    """1-based index of the background vertex nearest to each point."""
    ids = np.arange(1, m.np + 1) if among is None else np.asarray(among)
    v = m.xyz[ids]
    out = np.empty(len(x), np.int32)
    for a in range(0, len(x), 512):
        d = ((x[a:a + 512, None, :] - v[None, :, :]) ** 2).sum(-1)
        out[a:a + 512] = ids[np.argmin(d, axis=1)]
    return out


def run_pm(tr, m, x, t, sols, src, imet=0, flags=0, tets_mmg=None, pointmap=True, init=None, max_walk=0):
    tr.upload_background(m, sols, imet)
    tr.upload_points(x, t, tets_mmg=tets_mmg)
    tr.upload_point_sources(src)
    tr.run(flags=flags, record_starts=True, pointmap=pointmap, max_walk=max_walk)
    r = tr.download(init=init)
    e, v = tr.border()
    return r, tr.starts(), e, v


def check_parity(m, x, t, sols, src, r, edge, vert, imet=0, ref_t=None, init=None):
    """The oracle from the numpy starts against the device's results."""
    ref_t = t if ref_t is None else ref_t
    exp = expected_starts(m, t, src)
    o = O.Oracle(m)
    outs, elem, st, steps, e, v = o.interp(x, ref_t, sols, imet=imet, fresh=True, start_vol=exp,
                                           start_bdy=exp, init=init)
    bdy = np.nonzero(ref_t == M.TAG_BDY)[0]
    compare_exact((r.sols, r.elem, r.status, edge, vert), (outs, elem, st, e, v), bdy, len(sols))
    c = compare_volume(o, x, ref_t, (r.sols, r.elem, r.status), (outs, elem, st), sols)
    print(f"volume {c}, surface {len(bdy)}, oracle max |steps| {np.abs(steps).max()}, "
          f"exhaustive {(steps < 0).sum()}")
    assert c["same"] >= c["nvol"] - max(3, c["nvol"] // 1000)
    return exp, steps, st


@pytest.fixture(scope="module")
def case8():
    m, x, t, sols = cube_case(8, "iso")
    return m, x, t, sols, nearest_vertex(m, x)


def test_starts_are_the_reference(transfer, case8):
    m, x, t, sols, src = case8
    r, starts, _, _ = run_pm(transfer, m, x, t, sols, src)
    exp = expected_starts(m, t, src)
    assert np.all(r.status != 0)
    assert ((t & M.TAG_BDY) != 0).sum() > 0 and (t == 0).sum() > 0
    assert np.array_equal(starts, exp)
    # nearest-vertex sources are real starts, not the element-1 fallback
    assert (exp != 1).sum() > 0.9 * len(x)
    st = transfer.pointmap_stats()
    print(f"atomics: tets {st['atomics_tets']} of {4 * m.ne}, trias {st['atomics_trias']} of {3 * m.nt}")
    assert 0 < st["atomics_tets"] <= 4 * m.ne and 0 < st["atomics_trias"] <= 3 * m.nt


@pytest.mark.parametrize("n,metric,flags", [(8, "iso", 0), (9, "ani", FRESH), (10, "iso", REFWALK)])
def test_parity(transfer, n, metric, flags):
    m, x, t, sols = cube_case(n, metric)
    src = nearest_vertex(m, x)
    r, starts, edge, vert = run_pm(transfer, m, x, t, sols, src, flags=flags)
    exp, steps, st = check_parity(m, x, t, sols, src, r, edge, vert)
    assert np.array_equal(starts, exp)
    assert np.all(st == 1)


def test_far_sources(transfer, case8):
    """Sources far from their points: long walks, the surface walks' overflow
    passes and the exhaustive scans, all from point-map starts."""
    m, x, t, sols, _ = case8
    rng = np.random.default_rng(3)
    bv = np.unique(m.tria[1:].ravel())
    isb = (t & M.TAG_BDY) != 0
    src = np.where(isb, rng.choice(bv, size=len(x)), rng.integers(1, m.np + 1, size=len(x))).astype(np.int32)
    r, starts, edge, vert = run_pm(transfer, m, x, t, sols, src)
    exp, steps, st = check_parity(m, x, t, sols, src, r, edge, vert)
    assert np.array_equal(starts, exp)
    assert np.abs(steps).max() > 100 and (steps[isb] < 0).sum() > 0


def test_unset_sources(transfer, case8):
    m, x, t, sols, src0 = case8
    src = src0.copy()
    src[::3] = 0
    src[5::97] = m.np + 5
    src[7::101] = -4
    r, starts, edge, vert = run_pm(transfer, m, x, t, sols, src)
    exp, _, _ = check_parity(m, x, t, sols, src, r, edge, vert)
    unset = (src < 1) | (src > m.np)
    assert unset.sum() > len(x) // 3 and (src > m.np).sum() > 3
    assert np.array_equal(starts, exp)
    assert np.all(starts[unset] == 1)
    # exactly those: a set source starts from its own element (the few points
    # whose own source's element is element 1 left aside)
    own1 = expected_starts(m, t, src0) == 1
    assert own1.sum() < 20 and np.all(starts[~unset & ~own1] != 1)


def test_compaction_carries_the_source(transfer):
    """REQ and NUL points interleaved and a few orphans permute the lists:
    every located point must still start from ITS source's element."""
    n = 8
    m, x, t, sols = cube_case(n, "iso")
    t = t.copy()
    tets = M.new_point_tets(n, x, t)
    bi = np.nonzero((t & M.TAG_BDY) != 0)[0]
    orph = bi[3::53]                                   # a surface point's only tet is its own
    own = np.nonzero(np.isin(tets[:, 0], orph + 1))[0]
    tets[own, 0] = 0                                   # deleted new tets (!MG_EOK)
    t[5::7] |= M.TAG_REQ
    t[2::11] = M.TAG_NUL
    src = nearest_vertex(m, x)
    init = [np.full((len(x), s.shape[1]), -7.0) for s in sols]
    r, starts, edge, vert = run_pm(transfer, m, x, t, sols, src, flags=FRESH, tets_mmg=tets, init=init)
    ref_t = t.copy()
    ref_t[orph] = M.TAG_NUL                            # never visited: the oracle skips them too
    located = (ref_t == 0) | (ref_t == M.TAG_BDY)
    assert len(orph) > 3 and (~located).sum() > len(x) // 5 and (ref_t[orph] == M.TAG_NUL).all()
    exp, _, _ = check_parity(m, x, t, sols, src, r, edge, vert, ref_t=ref_t, init=init)
    assert np.array_equal(starts[located], exp[located])
    assert np.all(r.status[located] == 1)
    # the untouched rows stay as today
    assert np.all(r.elem[~located] == 0) and np.all(r.status[~located] == 0)
    assert np.all(starts[~located] == 0) and np.all(edge[~located] == -1) and np.all(vert[~located] == -1)
    for s in range(len(sols)):
        assert np.all(r.sols[s][~located] == -7.0)


def slit_cube(n=8):
    """Kuhn cube with a one-cell slit: the tets whose centroid has
    0.5 < x < 0.5 + 1/n and y < 0.75 removed."""
    m = M.kuhn_cube(n)
    c = m.centroids()
    cut = (c[:, 0] > 0.5) & (c[:, 0] < 0.5 + 1.0 / n) & (c[:, 1] < 0.75)
    return M.from_tets(m.xyz, np.concatenate([m.tet[:1], m.tet[1:][~cut]]))


def slit_points(npts=800, seed=6):
    rng = np.random.default_rng(seed)
    x = np.empty((npts, 3))
    x[: npts // 2, 0] = 0.48
    x[npts // 2:, 0] = 0.645
    x[:, 1] = rng.uniform(0.02, 0.73, npts)
    x[:, 2] = rng.uniform(0.02, 0.98, npts)
    return x


def test_nonconvex_slit(transfer):
    """Points beside the walls of a thin gap: the source vertex is connected
    to the point's side by construction.  nexhaust of this run and of a plain
    grid-start run are printed (recorded in DESIGN.md, not asserted)."""
    m = slit_cube(8)
    x = slit_points()
    t = np.zeros(len(x), np.uint16)
    sols = [M.on_vertices(m, M.iso_metric), M.on_vertices(m, lin_field)]
    src = nearest_vertex(m, x, among=np.unique(m.tet[1:].ravel()))
    r, starts, _, _ = run_pm(transfer, m, x, t, sols, src)
    pm_stats = transfer.locate_stats()
    exp = expected_starts(m, t, src)
    o = O.Oracle(m)
    outs, elem, st, steps, *_ = o.interp(x, t, sols, imet=0, fresh=True, start_vol=exp, start_bdy=exp)
    assert np.array_equal(starts, exp)
    assert np.all(st != 0), "the oracle itself must find every point"
    assert np.all(r.status != 0)
    c = compare_volume(o, x, t, (r.sols, r.elem, r.status), (outs, elem, st), sols)
    assert c["same"] >= c["nvol"] - max(3, c["nvol"] // 1000)
    transfer.run()                                      # the plain grid-start step on the same input
    grid_stats = transfer.locate_stats()
    print(f"slit: point-map nexhaust {pm_stats['nexhaust']} stepav {pm_stats['stepav']:.2f} "
          f"stepmax {pm_stats['stepmax']}; grid nexhaust {grid_stats['nexhaust']} "
          f"stepav {grid_stats['stepav']:.2f} stepmax {grid_stats['stepmax']}; "
          f"oracle exhaustive {(steps < 0).sum()} mean {np.abs(steps).mean():.2f}")


def test_refusals_and_lifetime(case8):
    m, x, t, sols, src = case8
    tr = Transfer(0)
    try:
        def plain_ok():
            tr.run()
            assert np.all(tr.download().status != 0)

        # sources before any points
        assert tr.lib.pmx_upload_point_sources(tr.ctx, src.ctypes.data_as(N.iptr), 4) == 0
        assert b"points" in tr.lib.pmx_last_error(tr.ctx)
        tr.upload_background(m, sols, 0)
        tr.upload_points(x, t, tets_mmg=M.new_point_tets(8, x, t))
        # the flag without sources
        with pytest.raises(RuntimeError, match="pmx_upload_point_sources"):
            tr.run(pointmap=True)
        plain_ok()
        tr.upload_point_sources(src)
        for seq in (N.RUN_SEQUENTIAL_SURFACE, N.RUN_SEQUENTIAL_VOLUME,
                    N.RUN_SEQUENTIAL_SURFACE | N.RUN_SEQUENTIAL_VOLUME):
            with pytest.raises(RuntimeError, match="SEQUENTIAL"):
                tr.run(pointmap=True, flags=seq)
            plain_ok()
        tr.run(pointmap=True)
        assert np.all(tr.download().status != 0)
        # forgotten on request, and by a new points upload
        tr.upload_point_sources(None)
        with pytest.raises(RuntimeError, match="pmx_upload_point_sources"):
            tr.run(pointmap=True)
        tr.upload_point_sources(src)
        tr.upload_points(x, t)
        with pytest.raises(RuntimeError, match="pmx_upload_point_sources"):
            tr.run(pointmap=True)
        plain_ok()
    finally:
        tr.close()


def _hint_grid(tr):
    g = np.zeros(1 << 22, np.int32)
    n = tr.lib.pmx_debug_hint_grid(tr.ctx, g.ctypes.data, len(g))
    assert 0 < n <= len(g)
    return g[:n]


def test_default_unchanged(transfer, case8):
    """Uploaded sources change nothing without the flag: fields, elements,
    status, edge, vertex and the surface starts bit for bit those of a context
    that never saw sources.

    The volume starts of a default step are the hint grid's, and k_hint_build
    fills a cell with a plain store (any sampled tet of the cell is a valid
    start, the last writer wins): they differ from run to run on the code
    before this feature too (measured: 2-3 of the 512 volume starts of this
    case between any two plain runs, same context or not, no sources
    anywhere), so no two runs can be compared on them.  What holds, and is
    checked, is that every volume start of the unflagged run is an entry of
    that run's own hint grid -- it was read from the grid, not from a source."""
    m, x, t, sols, src = case8
    ra, sa, ea, va = run_pm(transfer, m, x, t, sols, src, pointmap=False)
    ga = _hint_grid(transfer)
    tr = Transfer(0)
    try:
        tr.upload_background(m, sols, 0)
        tr.upload_points(x, t)
        tr.run(record_starts=True)
        rb = tr.download()
        eb, vb = tr.border()
        sb = tr.starts()
        gb = _hint_grid(tr)
    finally:
        tr.close()
    for a, b in zip(ra.sols, rb.sols):
        assert bits_equal(a, b).all()
    for a, b in ((ra.elem, rb.elem), (ra.status, rb.status), (ea, eb), (va, vb)):
        assert np.array_equal(a, b)
    isb = (t & M.TAG_BDY) != 0
    assert np.array_equal(sa[isb], sb[isb])
    assert ga.shape == gb.shape and (ga != 0).sum() > 0
    for s, g in ((sa, ga), (sb, gb)):
        assert np.all(np.isin(s[~isb], g[g != 0]) | (s[~isb] == 1))
    # and they are not the point-map starts
    assert (sa[~isb] != expected_starts(m, t, src)[~isb]).sum() > (~isb).sum() // 2


def test_seam_with_sources(transfer):
    """interp_metrics_and_fields with a "src" per group against the per-group
    point-map runs, bit for bit."""
    groups, want = [], []
    for n, metric in ((6, "iso"), (7, "iso")):
        m, x, t, sols = cube_case(n, metric)
        src = nearest_vertex(m, x)
        init = [np.full((len(x), s.shape[1]), -7.0) for s in sols]
        r, _, _, _ = run_pm(transfer, m, x, t, sols, src, init=init)
        want.append(r.sols)
        xyz1 = np.concatenate([np.zeros((1, 3)), x])
        tag1 = np.concatenate([np.zeros(1, np.uint16), t]).astype(np.uint16)
        src1 = np.concatenate([np.zeros(1, np.int32), src]).astype(np.int32)
        met = np.full((len(xyz1), sols[0].shape[1]), -7.0)
        fields = [np.full((len(xyz1), s.shape[1]), -7.0) for s in sols[1:]]
        groups.append(dict(old_mesh=m, old_met=sols[0], old_fields=sols[1:], xyz=xyz1, tags=tag1, met=met,
                           fields=fields, src=src1))
    tr = Transfer(0)
    try:
        assert tr.interp_metrics_and_fields(groups, input_met=1) == 1
    finally:
        tr.close()
    for g, w in zip(groups, want):
        got = [g["met"]] + g["fields"]
        for a, b in zip(got, w):
            assert np.isfinite(b).all() and not np.any(b == -7.0)
            assert bits_equal(a[1:], b).all()
