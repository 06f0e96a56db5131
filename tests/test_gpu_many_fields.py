"""GPU: any number of solution fields -- pmx_interp_more / Transfer.interp_more.

The fused step carries at most PMX_MAX_SOLS = 8 solutions; further fields are
interpolated in batches from the step's elements, without a second walk
(pmx_more.hip): a volume point's barycentrics are recomputed from (elem,
status, point), a surface point's were kept by the step.

The sharp check is the TWIN COLUMN: a field goes into the step and again as
one of the extra fields; the extra column must equal the step's column bit for
bit on every row, the untouched ones (init = -7) included.  It pins the
recomputed / stored barycentrics of every status class without a tolerance.
Beside it everything (step + extras) is compared with ONE oracle call over all
fields: surface rows with compare_exact, volume rows with compare_volume and
the cap the other suites use (same >= nvol - max(3, nvol // 1000)).
"""
import os

import numpy as np
import pytest

from conftest import REF_INPUTS
from helpers import bits_equal, compare_exact, compare_volume, cube_case, first_visit_order, lin_field
from oracle import oracle as O
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer
from test_gpu_pointmap import expected_starts, nearest_vertex, slit_cube

pytestmark = pytest.mark.gpu

FRESH = N.RUN_FRESH_BACKGROUND
REFWALK = N.RUN_REFERENCE_WALK
SEQ = N.RUN_SEQUENTIAL_SURFACE | N.RUN_SEQUENTIAL_VOLUME
SENT = -7.0
# (extra index, step column): the first three extras repeat step columns 1-3
# (a scalar, a vector, a tensor -- never the metric: on a surface vertex /
# edge hit the reference copies / 2-bar-interpolates the metric only)
TWINS = ((0, 1), (1, 2), (2, 3))


def spd_field(n1, rng):
    """Random symmetric positive definite tensors, Mmg's 6-component storage."""
    a = rng.normal(size=(n1, 3, 3))
    s = a @ a.transpose(0, 2, 1) + np.eye(3)
    return np.ascontiguousarray(np.stack([s[:, 0, 0], s[:, 0, 1], s[:, 0, 2], s[:, 1, 1], s[:, 1, 2], s[:, 2, 2]], 1))


def step_fields(m, metric, scalar, vector, rng):
    """The step's solutions: metric, a scalar, a vector, an SPD tensor."""
    return [metric, scalar, vector, spd_field(m.np + 1, rng)]


def extra_fields(m, step, nex, rng):
    """nex fields of sizes cycling 1, 3, 6 (size 6: SPD tensors, the others
    random); the first three are the twins of the step's columns 1, 2, 3."""
    out = []
    for k in range(nex):
        sz = (1, 3, 6)[k % 3]
        if k < 3:
            assert step[1 + k].shape[1] == sz
            out.append(step[1 + k].copy())
        elif sz == 6:
            out.append(spd_field(m.np + 1, rng))
        else:
            out.append(rng.normal(size=(m.np + 1, sz)))
    return out


def sent(n, sols):
    return [np.full((n, s.shape[1]), SENT) for s in sols]


def same_bits_or_nan(a, b):
    """Row-wise: every component has the same bits, or is NaN on both sides
    (a NaN's payload may depend on the order the compiler gives an addition's
    operands)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).reshape(a.shape[0], -1).all(axis=1)


def transfer_all(tr, m, x, t, step, extras, flags=0, tets=None, src=None, max_walk=0):
    """One step on `step` + interp_more on `extras`; every output starts at -7."""
    tr.upload_background(m, step, 0)
    tr.upload_points(x, t, tets_mmg=tets)
    if src is not None:
        tr.upload_point_sources(src)
    tr.run(flags=flags, record_starts=True, pointmap=src is not None, max_walk=max_walk)
    more = tr.interp_more(extras, init=sent(len(x), extras))     # the first consumer of the step's results
    r = tr.download(init=sent(len(x), step))
    e, v = tr.border()
    return r, more, tr.starts(), e, v


def check_twins(r, more, twins=TWINS):
    for ke, ks in twins:
        bad = ~bits_equal(more[ke], r.sols[ks])
        assert not bad.any(), f"extra {ke} != step column {ks} at rows {np.nonzero(bad)[0][:10]}"


def check_oracle(m, x, ref_t, step, extras, r, more, edge, vert, **kw):
    """Step + extras against one oracle call over all the fields."""
    allf = step + extras
    o = O.Oracle(m)
    outs, elem, st, steps, e, v = o.interp(x, ref_t, allf, imet=0, init=sent(len(x), allf), **kw)
    got = r.sols + more
    bdy = np.nonzero(ref_t == M.TAG_BDY)[0]
    if len(bdy):
        compare_exact((got, r.elem, r.status, edge, vert), (outs, elem, st, e, v), bdy, len(allf))
    c = compare_volume(o, x, ref_t, (got, r.elem, r.status), (outs, elem, st), allf)
    print(f"volume {c}, surface {len(bdy)}, {len(allf)} solutions")
    assert c["same"] >= c["nvol"] - max(3, c["nvol"] // 1000)
    return outs, elem, st, steps


# ---- 1. parity -----------------------------------------------------------------

@pytest.fixture(scope="module", params=[(6, "iso"), (7, "ani")], ids=["6iso", "7ani"])
def pcase(request):
    n, metric = request.param
    m, x, t, sols = cube_case(n, metric)
    rng = np.random.default_rng(100 + n)
    step = step_fields(m, sols[0], sols[1], sols[2], rng)
    extras = extra_fields(m, step, 19, rng)
    return n, m, x, t, step, extras


@pytest.mark.parametrize("mode", ["plain", "fresh", "refwalk", "seq"])
def test_parity(transfer, pcase, mode):
    n, m, x, t, step, extras = pcase
    assert [e.shape[1] for e in extras[:6]] == [1, 3, 6, 1, 3, 6] and len(extras) == 19
    flags = {"plain": 0, "fresh": FRESH, "refwalk": REFWALK, "seq": SEQ}[mode]
    tets = M.new_point_tets(n, x, t) if mode == "seq" else None
    r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras, flags=flags, tets=tets)
    assert ((t & M.TAG_BDY) != 0).sum() > 0 and (t == 0).sum() > 0 and np.all(r.status != 0)
    for a in more:
        assert not np.any(a == SENT) and np.isfinite(a).all()
    check_twins(r, more)
    if mode == "seq":
        check_oracle(m, x, t, step, extras, r, more, edge, vert, order=first_visit_order(tets, len(x)))
    else:
        check_oracle(m, x, t, step, extras, r, more, edge, vert, fresh=True, start_vol=starts, start_bdy=starts)
    assert transfer.kernel_ms(7) > 0.0                  # three batches' kernels, always recorded


def test_one_and_nine_fields(transfer, pcase):
    """One field (one batch, the 3-wide row); nine scalars (two batches: the
    8-wide row with 16-B loads, then one) -- against the 19-field call's twins
    and the oracle."""
    n, m, x, t, step, extras = pcase
    rng = np.random.default_rng(7)
    nine = [step[1].copy()] + [rng.normal(size=(m.np + 1, 1)) for _ in range(8)]
    transfer.upload_background(m, step, 0)
    transfer.upload_points(x, t)
    transfer.run(record_starts=True)
    r = transfer.download(init=sent(len(x), step))
    one = transfer.interp_more([step[2]], init=sent(len(x), [step[2]]))
    assert len(one) == 1 and bits_equal(one[0], r.sols[2]).all()
    got9 = transfer.interp_more(nine, init=sent(len(x), nine))
    assert len(got9) == 9 and bits_equal(got9[0], r.sols[1]).all()
    # a few more row widths of the scalar / vector form: 2, 4, 5, 6, 7
    for sizes in ((1, 1), (3, 1), (1, 3, 1), (3, 3), (3, 3, 1)):
        fl = [step[1] if sz == 1 else step[2] for sz in sizes]
        for a, sz in zip(transfer.interp_more(fl, init=sent(len(x), fl)), sizes):
            assert bits_equal(a, r.sols[1 if sz == 1 else 2]).all(), sizes
    e, v = transfer.border()
    starts = transfer.starts()
    check_oracle(m, x, t, step, nine, r, got9, e, v, fresh=True, start_vol=starts, start_bdy=starts)


# ---- 2. every status class -----------------------------------------------------

def test_closest_volume_and_surface(transfer):
    """(a) points pushed out of the cube, far point-map sources: the closest
    tet's one-hot (volume) and the exhaustive surface finishers."""
    m, x, t, sols = cube_case(8, "iso")
    rng = np.random.default_rng(3)
    bv = np.unique(m.tria[1:].ravel())
    isb = (t & M.TAG_BDY) != 0
    src = np.where(isb, rng.choice(bv, size=len(x)), rng.integers(1, m.np + 1, size=len(x))).astype(np.int32)
    x = x.copy()
    vol, bdy = np.nonzero(t == 0)[0], np.nonzero(isb)[0]
    x[vol[7::31][:16], 0] = 1.03
    x[bdy[3::29][:12]] += 0.2
    rng2 = np.random.default_rng(41)
    step = step_fields(m, sols[0], sols[1], sols[2], rng2)
    extras = extra_fields(m, step, 9, rng2)
    r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras, src=src)
    # the classes, on the device's own status
    assert (r.status[vol] == 0).sum() == 16 and (r.status[bdy] == 0).sum() == 12
    assert (r.status[bdy] == -1).sum() == 4
    assert np.all(r.elem[r.status == 0] > 0)
    check_twins(r, more)
    exp = expected_starts(m, t, src)
    check_oracle(m, x, t, step, extras, r, more, edge, vert, fresh=True, start_vol=exp, start_bdy=exp)


def test_surface_border_hits_and_exhaustive(transfer):
    """(b) wave.0.mesh, its own vertices moved by N(0, 2e-4): from own-vertex
    sources the surface walks end on edges and vertices (wedge / cone / border
    barycentrics); from far sources they end in the exhaustive scan (found
    and closest)."""
    m = M.read_medit(os.path.join(REF_INPUTS, "wave.0.mesh"))
    rng = np.random.default_rng(4)
    x = m.xyz[1:] + rng.normal(0.0, 2e-4, (m.np, 3))
    onb = np.zeros(m.np + 1, bool)
    onb[m.tria[1:].ravel()] = True
    t = np.where(onb[1:], M.TAG_BDY, 0).astype(np.uint16)
    isb = t != 0
    f = lambda p: (np.sin(3 * p[:, 0]) + p[:, 1])[:, None]  # noqa: E731
    vel = np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), np.cos(m.xyz[1:] * 2.0)]))
    rng2 = np.random.default_rng(42)
    step = step_fields(m, M.on_vertices(m, M.iso_metric), M.on_vertices(m, f), vel, rng2)
    extras = extra_fields(m, step, 9, rng2)
    own = np.arange(1, m.np + 1, dtype=np.int32)
    bv = np.unique(m.tria[1:].ravel())
    far = np.where(isb, rng.choice(bv, size=len(x)), rng.integers(1, m.np + 1, size=len(x))).astype(np.int32)
    for name, src in (("own", own), ("far", far)):
        r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras, src=src)
        if name == "own":
            assert (edge[isb] != -1).sum() == 78 and (vert[isb] != -1).sum() == 10
        else:
            assert (r.status[isb] == -1).sum() == 80 and (r.status[isb] == 0).sum() == 12
        check_twins(r, more)
        exp = expected_starts(m, t, src)
        check_oracle(m, x, t, step, extras, r, more, edge, vert, fresh=True, start_vol=exp, start_bdy=exp)


def test_volume_exhaustive(transfer):
    """(c) the slit cube: walks from sources anywhere in the mesh end stuck at
    the gap's walls and are found by the exhaustive scan (status -1)."""
    m = slit_cube(8)
    npts = 800
    rng = np.random.default_rng(6)
    x = np.empty((npts, 3))
    x[: npts // 2, 0] = 0.48
    x[npts // 2:, 0] = 0.645
    x[:, 1] = rng.uniform(0.02, 0.73, npts)
    x[:, 2] = rng.uniform(0.02, 0.98, npts)
    t = np.zeros(npts, np.uint16)
    src = rng.choice(np.unique(m.tet[1:].ravel()), size=npts).astype(np.int32)
    vel = np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), np.cos(m.xyz[1:] * 2.0)]))
    rng2 = np.random.default_rng(43)
    step = step_fields(m, M.on_vertices(m, M.iso_metric), M.on_vertices(m, lin_field), vel, rng2)
    extras = extra_fields(m, step, 9, rng2)
    r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras, src=src)
    check_twins(r, more)
    exp = expected_starts(m, t, src)
    _, _, st, _ = check_oracle(m, x, t, step, extras, r, more, edge, vert, fresh=True, start_vol=exp, start_bdy=exp)
    # the oracle's walk ends stuck for 295 of the 800 points.  The device's
    # volume walk is not the reference's step for step (and hands a walk longer
    # than max_walk to the scan too), so its own count is not that number: the
    # class must occur, and every point is found (no closest tet)
    assert (st == -1).sum() == 295
    nex = int((r.status == -1).sum())
    print(f"slit: device exhaustive {nex}, oracle 295")
    assert nex > 0 and np.all(np.abs(r.status) == 1)


# ---- 3. untouched rows ---------------------------------------------------------

@pytest.mark.parametrize("flags", [FRESH, 0], ids=["fresh", "default"])
def test_untouched_rows(transfer, flags):
    """REQ / NUL points, orphans (their only new tet deleted): the extra
    columns keep -7 exactly where the step leaves the rows alone -- the
    orphans classified by a FRESH step, or located and reset by the first
    consumer of a default step (here interp_more itself)."""
    n = 8
    m, x, t, sols = cube_case(n, "iso")
    t = t.copy()
    tets = M.new_point_tets(n, x, t)
    bi = np.nonzero((t & M.TAG_BDY) != 0)[0]
    orph = bi[3::53]
    own = np.nonzero(np.isin(tets[:, 0], orph + 1))[0]
    tets[own, 0] = 0                                   # deleted new tets (!MG_EOK)
    t[5::7] |= M.TAG_REQ
    t[2::11] = M.TAG_NUL
    src = nearest_vertex(m, x)
    rng = np.random.default_rng(44)
    step = step_fields(m, sols[0], sols[1], sols[2], rng)
    extras = extra_fields(m, step, 10, rng)
    r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras, flags=flags, tets=tets, src=src)
    ref_t = t.copy()
    ref_t[orph] = M.TAG_NUL                            # never visited: the oracle skips them too
    located = (ref_t == 0) | (ref_t == M.TAG_BDY)
    assert len(orph) > 3 and (~located).sum() > len(x) // 5
    assert np.all(r.elem[~located] == 0) and np.all(r.status[~located] == 0)
    for a in more:
        assert np.all(a[~located] == SENT)
        assert not np.any(a[located] == SENT)
    check_twins(r, more)
    exp = expected_starts(m, t, src)
    check_oracle(m, x, ref_t, step, extras, r, more, edge, vert, fresh=True, start_vol=exp, start_bdy=exp)


# ---- 4. singular tensors ---------------------------------------------------------

def test_singular_tensor(transfer):
    """Extra size-6 fields with tensors that do not invert at ~5 % of the
    vertices: the zero tensor (Mmg's diagonal branch inverts it to infinities:
    NaN rows, in the oracle too) and the rank-1 all-ones tensor (the
    inversion fails: PMMG_interp{3,4}bar_ani leave the row untouched,
    src/interpmesh_pmmg.c:258-267).  Exactly the rows the oracle leaves at init
    stay at init, for that field only; the batch's other fields are written."""
    m, x, t, sols = cube_case(6, "iso")
    rng = np.random.default_rng(11)
    zero = spd_field(m.np + 1, rng)
    zero[rng.random(m.np + 1) < 0.05] = 0.0
    ones = spd_field(m.np + 1, rng)
    ones[rng.random(m.np + 1) < 0.05] = 1.0
    step = [sols[0], sols[1], ones.copy()]
    extras = [rng.normal(size=(m.np + 1, 1)), zero, rng.normal(size=(m.np + 1, 3)), ones, spd_field(m.np + 1, rng)]
    r, more, starts, edge, vert = transfer_all(transfer, m, x, t, step, extras)
    allf = step + extras
    o = O.Oracle(m)
    outs, elem, st, *_ = o.interp(x, t, allf, imet=0, init=sent(len(x), allf), fresh=True, start_vol=starts,
                                  start_bdy=starts)
    got = r.sols + more
    same = elem == r.elem
    assert same.sum() >= len(x) - 3
    for k, (g, w) in enumerate(zip(got, outs)):
        ug, uw = (g == SENT).all(axis=1), (w == SENT).all(axis=1)
        assert np.array_equal(ug[same], uw[same]), f"solution {k}: untouched rows differ"
        assert np.array_equal(np.isnan(g)[same], np.isnan(w)[same]), f"solution {k}: NaN rows differ"
        fin = same & np.isfinite(w).all(axis=1)
        assert bits_equal(g[fin], w[fin]).all(), f"solution {k}"
    untouched = (more[3] == SENT).all(axis=1)
    assert 0 < untouched.sum() < len(x) // 2, "the all-ones tensors must leave rows untouched"
    assert np.isnan(more[1]).any() and not (more[1] == SENT).any()
    for k in (0, 2, 4):                                 # the same batch's other fields
        assert not np.any(more[k] == SENT) and np.isfinite(more[k]).all()
    # the twin of the step's singular column, untouched rows included
    assert same_bits_or_nan(more[3], r.sols[2]).all()
    assert np.array_equal((r.sols[2] == SENT).all(axis=1), untouched)


# ---- 5. refusals and lifetime ---------------------------------------------------

def test_refusals_and_lifetime():
    m, x, t, sols = cube_case(6, "iso")
    extras = [sols[1], sols[2]]
    tr = Transfer(0)
    try:
        def plain_ok():
            tr.run()
            assert np.all(tr.download().status != 0)

        with pytest.raises(RuntimeError, match="no step has run"):       # before any run
            tr.interp_more(extras)
        tr.upload_background(m, sols, 0)
        tr.upload_points(x, t)
        with pytest.raises(RuntimeError, match="no step has run"):
            tr.interp_more(extras)
        plain_ok()
        a = tr.interp_more(extras)
        b = tr.interp_more(extras)                                         # twice in a row
        r = tr.download()
        for u, v, w in zip(a, b, (r.sols[1], r.sols[2])):
            assert bits_equal(u, v).all() and bits_equal(u, w).all()
        tr.upload_points(x, t)                                             # points since the step
        with pytest.raises(RuntimeError, match="no step has run"):
            tr.interp_more(extras)
        plain_ok()
        tr.upload_background(m, sols, 0)                                   # background since the step
        with pytest.raises(RuntimeError, match="no step has run"):
            tr.interp_more(extras)
        plain_ok()
        with pytest.raises((RuntimeError, ValueError), match="rows"):      # wrong row count
            tr.interp_more([sols[1][:-3]])
        plain_ok()
        with pytest.raises((RuntimeError, ValueError)):
            tr.interp_more([])
        # the C ABI's own refusals: null and mismatched views
        ov, nv = (N.SolView * 1)(), (N.SolView * 1)()
        out = np.zeros((len(x), 1))
        ov[0].size, ov[0].m = 1, sols[1].ctypes.data_as(N.dptr)
        nv[0].size, nv[0].m = 3, out.ctypes.data_as(N.dptr)
        assert tr.lib.pmx_interp_more(tr.ctx, 1, ov, nv, len(x)) == 0
        assert b"mismatched" in tr.lib.pmx_last_error(tr.ctx)
        assert tr.lib.pmx_interp_more(tr.ctx, 1, None, nv, len(x)) == 0
        nv[0].size = 1
        assert tr.lib.pmx_interp_more(tr.ctx, 1, ov, nv, len(x) - 1) == 0
        assert b"capacity" in tr.lib.pmx_last_error(tr.ctx)
        assert np.all(out == 0.0)
        plain_ok()
        assert bits_equal(tr.interp_more(extras)[0], a[0]).all()
    finally:
        tr.close()


# ---- 6. the seam ------------------------------------------------------------------

@pytest.mark.parametrize("with_src", [False, True], ids=["grid", "src"])
def test_seam_many_fields(transfer, with_src):
    """interp_metrics_and_fields on two groups (alternating contexts), each
    with the metric and 11 fields, against the per-group run + interp_more,
    bit for bit."""
    groups, want = [], []
    for n, metric in ((6, "iso"), (7, "iso")):
        m, x, t, sols = cube_case(n, metric)
        rng = np.random.default_rng(200 + n)
        flds = [spd_field(m.np + 1, rng) if k % 3 == 2 else rng.normal(size=(m.np + 1, (1, 3, 6)[k % 3]))
                for k in range(11)]
        olds = [sols[0]] + flds
        src = nearest_vertex(m, x) if with_src else None
        r, more, *_ = transfer_all(transfer, m, x, t, olds[:8], olds[8:], src=src)
        want.append(r.sols + more)
        xyz1 = np.concatenate([np.zeros((1, 3)), x])
        tag1 = np.concatenate([np.zeros(1, np.uint16), t]).astype(np.uint16)
        g = dict(old_mesh=m, old_met=olds[0], old_fields=flds, xyz=xyz1, tags=tag1,
                 met=np.full((len(xyz1), 1), SENT), fields=[np.full((len(xyz1), f.shape[1]), SENT) for f in flds])
        if with_src:
            g["src"] = np.concatenate([np.zeros(1, np.int32), src]).astype(np.int32)
        groups.append(g)
    tr = Transfer(0)
    try:
        ier = tr.interp_metrics_and_fields(groups, input_met=1)
        assert ier == 1, tr.lib.pmx_last_error(tr.ctx).decode()
    finally:
        tr.close()
    for g, w in zip(groups, want):
        got = [g["met"]] + g["fields"]
        assert len(got) == 12
        for a, b in zip(got, w):
            assert np.isfinite(b).all() and not np.any(b == SENT)
            assert np.all(a[0] == SENT)                 # Mmg's slot 0 is not a point
            assert bits_equal(a[1:], b).all()


# ---- 7. the default step is unchanged ----------------------------------------------

def test_default_unchanged(transfer):
    """At most 8 solutions and no interp_more call: a context that served
    interp_more calls before gives, bit for bit, what a fresh context gives --
    fields, elements, status, edge, vertex and the surface starts (the volume
    starts are the hint grid's, a last-writer-wins table that differs from run
    to run: test_gpu_pointmap.test_default_unchanged)."""
    m, x, t, sols = cube_case(8, "iso")

    def plain(tr):
        tr.upload_background(m, sols, 0)
        tr.upload_points(x, t)
        tr.run(record_starts=True)
        r = tr.download()
        e, v = tr.border()
        return r, e, v, tr.starts()

    plain(transfer)
    transfer.interp_more([sols[1], sols[2]])            # this context's batch buffers exist
    ra, ea, va, sa = plain(transfer)
    tr = Transfer(0)
    try:
        rb, eb, vb, sb = plain(tr)
    finally:
        tr.close()
    assert len(ra.sols) == len(sols) <= 8
    for a, b in zip(ra.sols, rb.sols):
        assert bits_equal(a, b).all()
    for a, b in ((ra.elem, rb.elem), (ra.status, rb.status), (ea, eb), (va, vb)):
        assert np.array_equal(a, b)
    isb = (t & M.TAG_BDY) != 0
    assert isb.sum() > 0 and np.array_equal(sa[isb], sb[isb])
