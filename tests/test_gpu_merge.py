"""pmx_merge_groups / _fetch / _maps / _adopt on the GPU against the CPU twin
(tests/c/merge_ref.c): a rank's groups merged into one, PMMG_merge_grps
(reference src/mergemesh_pmmg.c:967-1073), and the merged group adopted as the
context's uploaded group.

Everything is compared for equality: the sizes, the eleven integer arrays of the
fetch, both maps of every group, and the xyz and solution rows bit for bit (they
are copies).  After an adopt, every later call is compared with the same call
on a second context that uploaded the fetched mesh.  No tolerance appears
anywhere.

The refusals that need more than 178 M tets or 2^31 points are not exercised."""
import ctypes as C

import numpy as np
import pytest

import merge_ref as R
import split_ref as S
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

SENT = R.SENT
PLAN_SLOT, FETCH_SLOT, ADOPT_SLOT = 16, 17, 18
CASES = R.cases()


def same_fetch(got, ref, data=True):
    for k in R.INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    if data:
        assert got["xyz"][1:].tobytes() == ref["xyz"][1:].tobytes()
        assert len(got["sols"]) == len(ref["sols"])
        for a, b in zip(got["sols"], ref["sols"]):
            assert a[1:].tobytes() == b[1:].tobytes()


def check_merge(tr, groups, comm, ref=None):
    """The device's merge equals the twin's: sizes, fetch, maps.  Returns the twin's."""
    ref = ref if ref is not None else R.merge(groups, comm)
    got = tr.merge_groups(groups, comm)
    assert np.array_equal(got["sizes"], ref["sizes"])
    same_fetch(tr.merge_fetch(), ref)
    for g in range(len(groups)):
        pn, tn = tr.merge_maps(g)
        assert pn.dtype == np.int32 and np.array_equal(pn, ref["maps"][g][0]), g
        assert tn.dtype == np.int32 and np.array_equal(tn, ref["maps"][g][1]), g
    return ref


def split_of(name):
    m, part, ngrp, sols = CASES[name]
    sp, comm = R.split_case(m, part, ngrp, sols)
    return m, sp["groups"], comm


# ---- 1. the round-trip cases ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_merge_equals_twin(transfer, name):
    m, groups, comm = split_of(name)
    ref = check_merge(transfer, groups, comm)
    assert (ref["sizes"][0], ref["sizes"][1]) == (m.np, m.ne)
    assert transfer.kernel_ms(PLAN_SLOT) > 0.0 and transfer.kernel_ms(FETCH_SLOT) > 0.0


def test_one_group(transfer):
    m = M.kuhn_cube(3)
    sp, comm = R.split_case(m, S.slabs(m, 2), 2, R.sols_of(m))
    g0 = sp["groups"][0]
    comm["ext_node"] = [g0["node_index2"][::-1].copy()]
    comm["ext_face"] = [g0["face_index2"][::-1].copy()]
    ref = check_merge(transfer, [g0], comm)
    assert np.array_equal(ref["tetra_v"], g0["tetra_v"])


# ---- 2. a remote group: external communicators ----------------------------------------------

@pytest.mark.parametrize("pieces", [1, 2])
def test_remote_group(transfer, pieces):
    m = M.kuhn_cube(6)
    part = S.fix_empty(np.random.default_rng(11).integers(0, 3, m.ne), 3)
    _, groups, comm, _ = R.remote_case(m, part, pieces, R.sols_of(m))
    if pieces == 2:      # the later communicator reuses positions of the first
        comm["ext_node"] = [comm["ext_node"][0], np.concatenate([comm["ext_node"][1], comm["ext_node"][0][:3]])]
    ref = check_merge(transfer, groups, comm)
    assert ref["sizes"][2] > 0 and ref["sizes"][3] > 0


def duplicate_case():
    m = M.kuhn_cube(3)
    _, groups, comm, _ = R.remote_case(m, S.slabs(m, 3), 1)
    g0, g1 = dict(groups[0]), dict(groups[1])
    free_n, free_f = comm["int_node_nitem"], comm["int_face_nitem"]
    comm = dict(comm, int_node_nitem=free_n + 2, int_face_nitem=free_f + 1)
    cat = lambda a, b: np.concatenate([a, b]).astype(np.int32)
    # group 0 names the new positions twice: the later entry stays
    g0["node_index1"], g0["node_index2"] = cat(g0["node_index1"], [1, 2]), cat(g0["node_index2"], [free_n, free_n])
    g0["face_index1"], g0["face_index2"] = cat(g0["face_index1"], [12, 27]), cat(g0["face_index2"], [free_f, free_f])
    # group 1 lists its first interface point again, at an empty position: that entry is dead
    g1["node_index1"] = cat(g1["node_index1"], g1["node_index1"][:1])
    g1["node_index2"] = cat(g1["node_index2"], [free_n + 1])
    comm["ext_node"] = [cat(comm["ext_node"][0], [free_n])]
    comm["ext_face"] = [cat(comm["ext_face"][0], [free_f])]
    return [g0, g1], comm, free_n


def test_duplicates_and_dead_entries(transfer):
    groups, comm, free_n = duplicate_case()
    ref = check_merge(transfer, groups, comm)
    assert ref["node_index1"][-1] == 2 and ref["face_index1"][-1] == 27
    # the dead entry created nothing: its position stays empty
    bad = dict(comm, ext_node=[np.array([free_n + 1], np.int32)])
    with pytest.raises(RuntimeError, match="no group filled"):
        transfer.merge_groups(groups, bad)


# ---- 3. determinism, partial fetches --------------------------------------------------------

def test_two_calls_identical_bytes(transfer):
    _, groups, comm = split_of("k6_random5")

    def run():
        sz = transfer.merge_groups(groups, comm)["sizes"]
        d = transfer.merge_fetch()
        blob = [sz.tobytes()] + [d[k].tobytes() for k in R.INT_KEYS] + [d["xyz"].tobytes()]
        blob += [a.tobytes() for a in d["sols"]]
        for g in range(len(groups)):
            blob += [a.tobytes() for a in transfer.merge_maps(g)]
        return b"".join(blob)

    assert run() == run()


def test_fetch_null_and_single_pointers(transfer):
    m = M.kuhn_cube(6)
    part = S.fix_empty(np.random.default_rng(11).integers(0, 3, m.ne), 3)
    _, groups, comm, _ = R.remote_case(m, part, 1, R.sols_of(m))
    transfer.merge_groups(groups, comm)
    full = transfer.merge_fetch()
    assert transfer.lib.pmx_merge_fetch(transfer.ctx, C.byref(N.MergeOut())) == 1
    for k in R.INT_KEYS + ("xyz",):
        a = np.full_like(full[k], SENT)
        o = N.MergeOut()
        setattr(o, k, a.ctypes.data_as(N.dptr if k == "xyz" else N.iptr))
        assert transfer.lib.pmx_merge_fetch(transfer.ctx, C.byref(o)) == 1
        body = slice(1, None) if k in ("xyz", "tetra_v") else slice(None)
        assert a[body].tobytes() == full[k][body].tobytes(), k
        if k in ("xyz", "tetra_v"):
            assert np.all(a[0] == SENT)                       # row 0 is the caller's
    assert np.array_equal(transfer.merge_maps(1)[0], R.merge(groups, comm)["maps"][1][0])
    assert transfer.lib.pmx_merge_maps(transfer.ctx, 0, None, None) == 1


# ---- 4. refusals ----------------------------------------------------------------------------

def raw_plan(tr, groups, comm, ngrp=None, nsol=None, null_groups=False, edit=None):
    gv, ns, c, meta, keep = tr._merge_views(groups, comm)
    if edit is not None:
        edit(gv, c)
    sz = N.MergeSizes(SENT, SENT, SENT, SENT)
    r = tr.lib.pmx_merge_groups(tr.ctx, len(groups) if ngrp is None else ngrp, None if null_groups else gv,
                                ns if nsol is None else nsol, C.byref(c), C.byref(sz))
    clean = (sz.np, sz.ne, sz.nnode, sz.nface) == (SENT,) * 4
    return r, clean, tr.lib.pmx_last_error(tr.ctx)


def raw_fetch(tr, n=64):
    arr = {k: np.full(n, SENT, np.int32) for k in R.INT_KEYS}
    xyz = np.full(n, float(SENT))
    o = N.MergeOut()
    for k, a in arr.items():
        setattr(o, k, a.ctypes.data_as(N.iptr))
    o.xyz = xyz.ctypes.data_as(N.dptr)
    r = tr.lib.pmx_merge_fetch(tr.ctx, C.byref(o))
    clean = all(np.all(a == SENT) for a in arr.values()) and np.all(xyz == SENT)
    return r, clean, tr.lib.pmx_last_error(tr.ctx)


def test_refusals_leave_outputs_untouched(transfer):
    m = M.kuhn_cube(3)
    _, groups, comm, _ = R.remote_case(m, S.slabs(m, 3), 1, R.sols_of(m))
    tr = Transfer(0)
    try:
        r, clean, err = raw_fetch(tr)
        assert r == 0 and clean and b"no plan" in err
        pn = np.full(8, SENT, np.int32)
        assert tr.lib.pmx_merge_maps(tr.ctx, 0, pn.ctypes.data_as(N.iptr), None) == 0 and np.all(pn == SENT)
        assert tr.lib.pmx_merge_adopt(tr.ctx, 0) == 0 and b"no plan" in tr.lib.pmx_last_error(tr.ctx)
        assert all(tr.kernel_ms(s) == -1.0 for s in (PLAN_SLOT, FETCH_SLOT, ADOPT_SLOT))
    finally:
        tr.close()

    def refused(what, g=None, c=None, **kw):
        # a good plan first: the refused call must not leave it behind either
        transfer.merge_groups(groups, comm)
        r, clean, err = raw_plan(transfer, g if g is not None else groups, c if c is not None else comm, **kw)
        assert r == 0 and clean and what in err, err
        assert transfer.kernel_ms(PLAN_SLOT) == -1.0
        r, clean, err = raw_fetch(transfer)
        assert r == 0 and clean and b"no plan" in err

    def with_group(i, **arrays):
        g = [dict(d) for d in groups]
        g[i].update(arrays)
        return g

    def edited(i, key, at, value):
        a = np.array(groups[i][key], np.int32)
        a[at] = value
        return with_group(i, **{key: a})

    np1, ne1 = groups[1]["xyz"].shape[0] - 1, groups[1]["tetra_v"].shape[0] - 1
    nn, nf = comm["int_node_nitem"], comm["int_face_nitem"]
    refused(b"ngrp < 1", ngrp=0)
    refused(b"groups is NULL", null_groups=True)
    refused(b"NULL view", edit=lambda gv, c: setattr(gv[1], "point_c", None))
    refused(b"NULL view", edit=lambda gv, c: setattr(gv[0], "tetra_v", None))
    refused(b"NULL view", edit=lambda gv, c: setattr(gv[1], "node_index2", None))
    refused(b"NULL view", edit=lambda gv, c: setattr(c, "node_items", None))
    refused(b"deleted tet", edited(1, "tetra_v", (5, 0), 0))
    refused(b"vertex outside 1..np", edited(1, "tetra_v", (5, 2), np1 + 1))
    refused(b"vertex outside 1..np", edited(0, "tetra_v", (7, 3), 0))
    refused(b"nsol outside", nsol=9)
    refused(b"nsol outside", nsol=-1)
    refused(b"sizes differ", with_group(1, sols=[groups[1]["sols"][0], groups[1]["sols"][0]]))
    refused(b"point outside 1..np", edited(1, "node_index1", 0, 0))
    refused(b"point outside 1..np", edited(1, "node_index1", -1, np1 + 1))
    refused(b"position outside 0..int_node_nitem-1", edited(0, "node_index2", 0, nn))
    refused(b"position outside 0..int_node_nitem-1", edited(1, "node_index2", 0, -1))
    refused(b"outside 12..12*ne+11", edited(1, "face_index1", 0, 11))
    refused(b"outside 12..12*ne+11", edited(1, "face_index1", 0, 12 * ne1 + 12))
    refused(b"position outside 0..int_face_nitem-1", edited(0, "face_index2", 0, nf))
    ext = lambda kind, at, v: dict(comm, **{"ext_" + kind: [np.concatenate([comm["ext_" + kind][0][:at], [v],
                                                                             comm["ext_" + kind][0][at + 1:]])]})
    refused(b"external node item out of range", c=ext("node", 0, nn))
    refused(b"external face item out of range", c=ext("face", 0, -1))
    refused(b"no group filled", c=dict(ext("node", 0, nn), int_node_nitem=nn + 1))
    refused(b"no group filled", c=dict(ext("face", 0, nf), int_face_nitem=nf + 1))
    refused(b"appears twice", c=ext("node", 1, int(comm["ext_node"][0][0])))
    # the context is usable: a correct call right after succeeds
    check_merge(transfer, groups, comm)
    with pytest.raises(RuntimeError, match="solution"):
        saved = transfer._merge["sol_sizes"]
        transfer._merge["sol_sizes"] = [3, 3]
        try:
            transfer.merge_fetch()
        finally:
            transfer._merge["sol_sizes"] = saved
    for g in (-1, 2):
        pn = np.full(8, SENT, np.int32)
        assert transfer.lib.pmx_merge_maps(transfer.ctx, g, pn.ctypes.data_as(N.iptr), None) == 0
        assert np.all(pn == SENT) and b"out of range" in transfer.lib.pmx_last_error(transfer.ctx)
    assert transfer.lib.pmx_merge_adopt(transfer.ctx, 2) == 0 and b"imet" in transfer.lib.pmx_last_error(transfer.ctx)
    # an upload leaves the plan alone; a release drops it
    transfer.upload_background(m, [np.ones((m.np + 1, 1))], 0)
    same_fetch(transfer.merge_fetch(), R.merge(groups, comm))
    transfer.merge_release()
    r, clean, err = raw_fetch(transfer)
    assert r == 0 and clean and b"no plan" in err
    assert all(transfer.kernel_ms(s) == -1.0 for s in (PLAN_SLOT, FETCH_SLOT, ADOPT_SLOT))


# ---- 5. timers ------------------------------------------------------------------------------

def test_timers():
    _, groups, comm = split_of("k3_slabs2")
    tr = Transfer(0)
    try:
        assert all(tr.kernel_ms(s) == -1.0 for s in (PLAN_SLOT, FETCH_SLOT, ADOPT_SLOT))
        tr.merge_groups(groups, comm)
        assert tr.kernel_ms(PLAN_SLOT) > 0.0 and tr.kernel_ms(FETCH_SLOT) == -1.0 and tr.kernel_ms(ADOPT_SLOT) == -1.0
        tr.merge_fetch()
        assert tr.kernel_ms(FETCH_SLOT) > 0.0 and tr.kernel_ms(ADOPT_SLOT) == -1.0
        tr.merge_adopt(0)
        assert tr.kernel_ms(ADOPT_SLOT) > 0.0
    finally:
        tr.close()


# ---- 6. adopt -------------------------------------------------------------------------------

def bare_mesh(d):
    """The fetched group as a mesh without trias and without Mmg's adjacency."""
    ne = d["tetra_v"].shape[0] - 1
    return M.Mesh(d["xyz"], d["tetra_v"], np.zeros(4 * ne + 5, np.int32), np.zeros((1, 3), np.int32),
                  np.zeros(4, np.int32))


def stray_partition(mm, nparts):
    """x-slabs with a few tets of the last slab recoloured deep inside the first."""
    part = S.x_slabs(mm, nparts)
    x = mm.centroids()[:, 0]
    part[np.argsort(x)[:3]] = nparts - 1
    return part


@pytest.mark.parametrize("name", ["k3_slabs3", "k6_slabs8"])
def test_adopt_equals_upload(transfer, name):
    m, groups, comm = split_of(name)
    ref = check_merge(transfer, groups, comm)
    transfer.merge_adopt(0)
    assert transfer.kernel_ms(ADOPT_SLOT) > 0.0
    d = transfer.merge_fetch()
    same_fetch(d, ref)                                        # the plan survives the adopt
    mm = bare_mesh(d)
    other = Transfer(0)
    try:
        other.upload_background(mm, d["sols"], 0, adja=False)
        both = (transfer, other)
        for w in (True, False):
            a, b = (t.metis_graph(weights=w) for t in both)
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(x, y)
        part = S.x_slabs(mm, 3)
        a, b = (t.contiguity(part, 3) for t in both)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        stray = stray_partition(mm, 3)
        (pa, sa), (pb, sb) = (t.fix_contiguity(stray, 3) for t in both)
        assert np.array_equal(pa, pb) and sa["nmerged"] >= 1
        for k in ("ncomp", "nmerged", "nmerged_tets", "ncannot", "counter"):
            assert sa[k] == sb[k], k
        a, b = (t.split_groups(pa, 3) for t in both)
        assert np.array_equal(a["sizes"], b["sizes"]) and np.array_equal(a["tet_new"], b["tet_new"])
        assert (a["int_face_nitem"], a["int_node_nitem"]) == (b["int_face_nitem"], b["int_node_nitem"])
        for g in range(3):
            ga, gb = (t.split_fetch(g) for t in both)
            for k in S.INT_KEYS:
                assert np.array_equal(ga[k], gb[k]), k
            assert ga["xyz"][1:].tobytes() == gb["xyz"][1:].tobytes()
            for x, y in zip(ga["sols"], gb["sols"]):
                assert x[1:].tobytes() == y[1:].tobytes()
        pts = np.random.default_rng(5).uniform(0.05, 0.95, (300, 3))
        res = []
        for t in both:
            t.upload_points(pts, np.zeros(len(pts), np.uint16))
            t.run()
            res.append(t.download())
        assert np.array_equal(res[0].elem, res[1].elem) and np.array_equal(res[0].status, res[1].status)
        assert np.all(res[0].status != 0)
        for x, y in zip(res[0].sols, res[1].sols):
            assert x.tobytes() == y.tobytes()
        same_fetch(transfer.merge_fetch(), ref)
    finally:
        other.close()
        transfer.merge_release()


def test_adopt_then_fresh_step(transfer):
    """A FRESH step on an adopted group matches its faces and builds its tet
    records again from the connectivity the adopt kept: same bytes as the
    default step before it and after it."""
    _, groups, comm = split_of("k6_slabs8")
    transfer.merge_groups(groups, comm)
    try:
        transfer.merge_adopt(0)
        pts = np.random.default_rng(7).uniform(0.05, 0.95, (300, 3))
        transfer.upload_points(pts, np.zeros(len(pts), np.uint16))
        res = []
        for flags in (0, N.RUN_FRESH_BACKGROUND, 0):
            transfer.run(flags=flags)
            res.append(transfer.download())
        assert np.all(res[0].status != 0)
        for r in res[1:]:
            assert np.array_equal(r.elem, res[0].elem) and np.array_equal(r.status, res[0].status)
            for x, y in zip(r.sols, res[0].sols):
                assert x.tobytes() == y.tobytes()
    finally:
        transfer.merge_release()


def test_adopt_glued_cubes(transfer):
    m, groups, comm = split_of("glued")
    ref = check_merge(transfer, groups, comm)
    transfer.merge_adopt(0)
    d = transfer.merge_fetch()
    other = Transfer(0)
    try:
        other.upload_background(bare_mesh(d), d["sols"], 0, adja=False)
        a, b = (t.contiguity() for t in (transfer, other))
        assert a[0] == b[0] == 2 and np.array_equal(a[2], b[2])
        a, b = (t.metis_graph(weights=False) for t in (transfer, other))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        other.close()


def test_adopt_refuses_non_manifold_faces(transfer):
    """Three tets on one face: the adopt fails as the upload does, and no background is left."""
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [1, 1, -1]], np.float64)
    tv = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [1, 3, 2, 5], [1, 3, 2, 6]], np.int32)
    grp = {"tetra_v": tv, "xyz": xyz, "sols": [np.ones((7, 1))]}
    tr = Transfer(0)
    try:
        tr.upload_background(M.kuhn_cube(2), [np.ones((M.kuhn_cube(2).np + 1, 1))], 0)
        tr.merge_groups([grp])
        with pytest.raises(RuntimeError, match="non-manifold"):
            tr.merge_adopt(0)
        with pytest.raises(RuntimeError):
            tr.metis_graph(weights=False)                     # no background
        assert np.array_equal(tr.merge_fetch()["tetra_v"], tv)
        with pytest.raises(RuntimeError, match="non-manifold"):
            tr.upload_background(bare_mesh(tr.merge_fetch()), [np.ones((7, 1))], 0, adja=False)
    finally:
        tr.close()


# ---- 7. lifecycle ---------------------------------------------------------------------------

def test_plan_adopt_release_destroy_leave_nothing_behind(transfer):
    _, groups, comm = split_of("k3_slabs3")
    lib = N.load()
    before = lib.pmx_debug_live_allocations()
    for refuse in (False, True):
        tr = Transfer(0)
        try:
            if refuse:
                bad = [dict(d) for d in groups]
                bad[1]["tetra_v"] = bad[1]["tetra_v"].copy()
                bad[1]["tetra_v"][3, 0] = 0
                with pytest.raises(RuntimeError, match="deleted tet"):
                    tr.merge_groups(bad, comm)
            else:
                tr.merge_groups(groups, comm)
                assert lib.pmx_debug_live_allocations() > before
                tr.merge_adopt(0)
                tr.merge_fetch()
                tr.merge_release()
        finally:
            tr.close()
        assert lib.pmx_debug_live_allocations() == before
    # and a plan that its context's destruction frees
    tr = Transfer(0)
    tr.merge_groups(groups, comm)
    tr.close()
    assert lib.pmx_debug_live_allocations() == before
