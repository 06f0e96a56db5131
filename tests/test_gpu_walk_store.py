"""The volume walk's result rows: block stores against per-lane stores.

`k_walks` stores the rows of a wave whose 64 points are consecutive volume
points with rows of their own as one block through LDS, and every other wave
lane by lane.  `k_walk` (PMX_RUN_REFERENCE_WALK) kept its per-lane epilogue and
is the device reference here: every case runs the step twice on one upload,
as is and with the reference walk, and every array the step returns must be
the same bit for bit -- fields (unwritten rows keep the sentinel, so the write
masks are covered), elements, status, the border arrays, the locate and wave
counts.

Step counts and start tets are compared where the two steps started a point
from the same tet: several sampled tets can share a hint cell and the last
store wins, so a start (and the number of steps from it) may differ between
any two steps, whatever the kernel (tests/test_gpu_edge_cases.py,
test_fresh_step_equals_upload_step).  Their signs (located / stuck / never
visited) are compared everywhere.

Sizes: kuhn_cube(6..8), 216 / 343 / 512 volume points -- 4 to 8 waves in two
workgroups, the last wave partial unless the count is 512.
"""
import functools

import numpy as np
import pytest

from parmmg_amd import _native as N
from parmmg_amd import mesh as M

pytestmark = pytest.mark.gpu

REFWALK = N.RUN_REFERENCE_WALK
NOTIES = N.RUN_NO_INLINE_TIES
FRESH = N.RUN_FRESH_BACKGROUND
SENT = -7.0

# solution sizes per row width S (scalars and vectors; the first scalar is the metric)
ISO_SIZES = {1: [1], 2: [1, 1], 3: [3], 4: [1, 3], 5: [1, 1, 3], 6: [3, 3], 7: [1, 3, 3], 8: [1, 1, 3, 3]}


@functools.lru_cache(maxsize=None)
def cube(n):
    m = M.kuhn_cube(n)
    x, t = M.new_points(n, surface=False)
    assert len(x) == n ** 3 and not t.any()
    return m, x, t


def iso_sols(m, sizes, seed=11):
    rng = np.random.default_rng(seed)
    sols = [rng.uniform(0.5, 1.5, (m.np + 1, s)) for s in sizes]
    return sols, (0 if sizes[0] == 1 else -1)


def ani_sols(m):
    return [M.on_vertices(m, M.shock_metric)], 0


def interior_tets(m, count, seed=2):
    """Tets with four interior neighbours."""
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4)
    ks = np.nonzero((nb != 0).all(axis=1))[0] + 1
    return np.random.default_rng(seed).choice(ks, count, replace=False)


def both(tr, m, x, t, sols, imet, tets=None, flags=0, **run):
    """The step as is and with the reference walk, on one upload."""
    n = len(x)
    tr.upload_background(m, sols, imet)
    tr.upload_points(x, t, tets)
    res = []
    for f in (flags, flags | REFWALK):
        tr.run(flags=f, record_starts=True, **run)
        r = tr.download(init=[np.full((n, s.shape[1]), SENT) for s in sols])
        res.append(dict(r=r, starts=tr.starts().copy(), border=tr.border(), locate=tr.locate_stats(),
                        waves=tr.wave_stats(0)))
    return res


def assert_same(a, b, what="", capped=False):
    """capped: the walk's step cap is small, so whether a point is located by
    its walk or by the exhaustive scan (status 1 / -1, the sign of steps)
    depends on its start too; the located tet and the fields do not."""
    ra, rb = a["r"], b["r"]
    same = a["starts"] == b["starts"]
    assert same.mean() > 0.5, what
    cmp = same if capped else np.ones(len(same), bool)
    for k, (u, v) in enumerate(zip(ra.sols, rb.sols)):
        bad = np.nonzero((u.view(np.uint64) != v.view(np.uint64)).any(axis=1))[0]
        assert bad.size == 0, f"{what}: solution {k} differs in rows {bad[:8]} ({bad.size})"
    assert np.array_equal(ra.elem, rb.elem), what
    assert np.array_equal(ra.status[cmp], rb.status[cmp]), what
    assert np.array_equal(ra.status == 0, rb.status == 0), what
    assert np.array_equal(a["border"][0], b["border"][0]) and np.array_equal(a["border"][1], b["border"][1]), what
    assert np.array_equal(np.sign(ra.steps)[cmp], np.sign(rb.steps)[cmp]), what
    assert np.array_equal(ra.steps[same], rb.steps[same]), what
    for f in ("nvol", "nbdy", "nclosest") + (("nexhaust",) if cmp.all() else ()):
        assert a["locate"][f] == b["locate"][f], (what, f)
    for f in ("waves", "located"):
        if cmp.all():
            assert a["waves"][f] == b["waves"][f], (what, f)
    if same.all():
        for f in ("stepmin", "stepmax", "stepav"):
            assert a["locate"][f] == b["locate"][f], (what, f)
        for f in ("step_sum", "lane_steps", "wave_max_hist"):
            assert a["waves"][f] == b["waves"][f], (what, f)


@pytest.mark.parametrize("n", [8, 7])
@pytest.mark.parametrize("S", sorted(ISO_SIZES))
def test_contiguous_windows_iso(transfer, S, n):
    """All points volume points: every full wave's rows are one block.
    n = 8: 512 points, full waves only; n = 7: 343, the last wave partial."""
    m, x, t = cube(n)
    sols, imet = iso_sols(m, ISO_SIZES[S])
    a, b = both(transfer, m, x, t, sols, imet)
    assert_same(a, b, f"S={S} n={n}")
    assert (a["r"].status == 1).all() and not any((s == SENT).any() for s in a["r"].sols)
    assert a["waves"]["waves"] == -(-len(x) // 64) and a["waves"]["located"] == len(x)


@pytest.mark.parametrize("n", [8, 7])
def test_contiguous_windows_ani(transfer, n):
    m, x, t = cube(n)
    sols, imet = ani_sols(m)
    a, b = both(transfer, m, x, t, sols, imet)
    assert_same(a, b, f"ani n={n}")
    assert (a["r"].status == 1).all() and not (a["r"].sols[0] == SENT).any()


def test_ani_singular_row_writes_nothing(transfer):
    """A background vertex with a rank-one metric: the inversion fails for
    every point located in a tet around it, those lanes write nothing (the
    reference leaves the output untouched) inside otherwise consecutive waves."""
    m, x, t = cube(8)
    sols, imet = ani_sols(m)
    sols = [sols[0].copy()]
    k = interior_tets(m, 3, seed=9)
    sols[0][m.tet[k, 0]] = 1.0                       # det = 0, off-diagonal above MMG5_EPS
    a, b = both(transfer, m, x, t, sols, imet)
    assert_same(a, b, "singular")
    r = a["r"]
    kept = (r.sols[0] == SENT).all(axis=1)
    assert (r.status == 1).all() and 0 < kept.sum() < 64
    assert np.isin(m.tet[r.elem[kept]], m.tet[k, 0]).any(axis=1).all()
    assert not (r.sols[0][~kept] == SENT).any()


@pytest.mark.parametrize("layout", ["iso5", "ani"])
@pytest.mark.parametrize("stride", [65, 63])
def test_windows_with_tag_holes(transfer, stride, layout):
    """Every stride-th point a boundary, required or NUL point in turn: the
    volume list skips it, so the window around it is not consecutive."""
    m, x, t = cube(8)
    sols, imet = iso_sols(m, ISO_SIZES[5]) if layout == "iso5" else ani_sols(m)
    t = t.copy()
    holes = np.arange(1, len(x), stride)
    t[holes] = np.resize(np.array([M.TAG_BDY, M.TAG_REQ, M.TAG_NUL], np.uint16), len(holes))
    a, b = both(transfer, m, x, t, sols, imet)
    assert_same(a, b, f"stride={stride} {layout}")
    r = a["r"]
    assert (r.status[t == 0] == 1).all() and a["locate"]["nvol"] == (t == 0).sum()
    skip = (t == M.TAG_REQ) | (t == M.TAG_NUL)
    assert all((s[skip] == SENT).all() and not (s[t == 0] == SENT).any() for s in r.sols)


@pytest.mark.parametrize("flags", [0, FRESH])
def test_windows_with_orphans(transfer, flags):
    """New tets that leave points out: orphans are never located; marked at
    the upload (flags 0) and inside the FRESH step."""
    m, x, t = cube(7)
    sols, imet = iso_sols(m, ISO_SIZES[5])
    n = len(x)
    rng = np.random.default_rng(4)
    used = rng.random(n) < 0.9
    pool = np.nonzero(used)[0]
    tets = np.zeros((len(pool) + 1, 4), np.int32)
    tets[1:] = rng.choice(pool, size=(len(pool), 4))
    tets[1:, 0] = pool
    tets[0] = -1
    a, b = both(transfer, m, x, t, sols, imet, tets=tets, flags=flags)
    assert_same(a, b, f"orphans flags={flags}")
    r = a["r"]
    assert (r.status[used] == 1).all() and (r.status[~used] == 0).all() and (r.elem[~used] == 0).all()
    assert all((s[~used] == SENT).all() and not (s[used] == SENT).any() for s in r.sols)


@pytest.mark.parametrize("flags", [0, NOTIES])
def test_tie_lanes(transfer, flags):
    """Old vertices, edge midpoints and face centroids of interior tets inside
    otherwise consecutive waves: resolved in place or handed to the tie list."""
    m, x, t = cube(8)
    sols, imet = iso_sols(m, ISO_SIZES[5])
    P = m.xyz[m.tet[interior_tets(m, 9)]]
    x = x.copy()
    at = np.array([3, 70, 77, 140, 200, 260, 330, 400, 511])
    x[at[:3]] = P[:3, 0]
    x[at[3:6]] = 0.5 * (P[3:6, 0] + P[3:6, 1])
    x[at[6:]] = P[6:, :3].mean(axis=1)
    a, b = both(transfer, m, x, t, sols, imet, flags=flags)
    assert_same(a, b, f"ties flags={flags}")
    assert (a["r"].status == 1).all() and not any((s == SENT).any() for s in a["r"].sols)
    assert a["waves"]["located"] < len(x)            # the tie list took some


@pytest.mark.parametrize("max_walk", [0, 3])
def test_stuck_lanes(transfer, max_walk):
    """Points outside the mesh (and, with max_walk = 3, every longer walk) go
    to the stuck list; their lanes have no row."""
    m, x, t = cube(8)
    sols, imet = iso_sols(m, ISO_SIZES[5])
    x = x.copy()
    out = np.array([5, 130, 447])
    x[out] = [[1.5, -0.5, 0.5], [0.5, 0.5, 1.25], [-0.125, 0.5, 0.5]]
    a, b = both(transfer, m, x, t, sols, imet, max_walk=max_walk)
    assert_same(a, b, f"stuck max_walk={max_walk}", capped=max_walk > 0)
    r = a["r"]
    inside = np.ones(len(x), bool)
    inside[out] = False
    assert (r.status[out] == 0).all() and (r.status[inside] != 0).all()
    assert a["locate"]["nexhaust"] >= len(out) and a["waves"]["located"] <= len(x) - len(out)


def test_constant_size_metric(transfer):
    """-hsiz: the metric is set, not interpolated -- the generic layout, whose
    rows are stored lane by lane."""
    m, x, t = cube(7)
    sols, imet = iso_sols(m, ISO_SIZES[5])
    a, b = both(transfer, m, x, t, sols, imet, hsiz=0.05)
    assert_same(a, b, "hsiz")
    r = a["r"]
    assert (r.status == 1).all() and (r.sols[0] == 0.05).all()
    assert not any((s == SENT).any() for s in r.sols[1:])


@pytest.mark.parametrize("S", [1, 3, 5, 7])
def test_odd_first_index(transfer, S):
    """Point 0 is no volume point: the waves start at odd point indices, and
    with S odd their blocks at addresses that are 8-B but not 16-B aligned."""
    m, x, t = cube(8)
    sols, imet = iso_sols(m, ISO_SIZES[S])
    t = t.copy()
    t[0] = M.TAG_NUL
    a, b = both(transfer, m, x, t, sols, imet)
    assert_same(a, b, f"odd i0 S={S}")
    r = a["r"]
    assert (r.status[1:] == 1).all() and r.status[0] == 0
    assert all((s[0] == SENT).all() and not (s[1:] == SENT).any() for s in r.sols)
