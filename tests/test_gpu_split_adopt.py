"""pmx_split_adopt / pmx_download_surface: one group of a split plan becomes
another context's background on the device, volume and surface (the new group
of PMMG_split_n2mGrps as PMMG_update_oldGrps' next background, reference
src/libparmmg1.c:653, with MMG5_chkBdryTria + MMG3D_hashTria,
src/grpsplit_pmmg.c:400-414).

Every comparison is equality of bytes; no tolerance appears.  The partner of
every comparison is a second context that uploads the mesh the CPU builders
make of the fetched group (split_ref.group_mesh, i.e. mesh.from_tets) with the
fetched solution rows and adja=False.

The points of a step are new_points(n) of the whole cube plus one MG_BDY point
at the centroid of every new interface face of the group.  A point outside the
group cannot be located in it: it takes the closest element and status 0 by
definition (the CPU oracle locates 6 to 99 of the 81 to 432 cube points per
group), so "located" is asserted for every point the CPU oracle locates on the
same inputs (fresh queries from the uploading context's start trias, the
convention of test_gpu_parity.py) -- the interface centroids all among them --
and the bytes are compared for every point.

The refusal "contexts on different devices" is not exercised: one GPU cannot
produce it."""
import numpy as np
import pytest

import split_ref as S
from oracle.oracle import Oracle
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

gpu = pytest.mark.gpu

SENT = -77
ADOPT_SLOT = 21


def sols_of(m):
    return [M.on_vertices(m, M.iso_metric), M.on_vertices(m, M.velocity)]


def case(name):
    """(mesh, part, ngrp, n of new_points)"""
    if name == "k3_slabs3":
        m = M.kuhn_cube(3)
        return m, S.slabs(m, 3), 3, 3
    if name == "wave_xslabs4":
        m = S.wave_mesh()
        return m, S.x_slabs(m, 4), 4, 4
    m = M.kuhn_cube(6)
    if name == "k6_slabs6":                 # one component each, closed manifold surfaces: k_fan_rotate
        return m, S.slabs(m, 6), 6, 6
    if name == "k6_slabs8":                 # thinner than a cell: pieces that touch along edges and vertices
        return m, S.slabs(m, 8), 8, 6
    assert name == "k6_random5"             # a ragged interface
    return m, S.fix_empty(np.random.default_rng(7).integers(0, 5, m.ne), 5), 5, 6


CASES = ["k3_slabs3", "k6_slabs6", "k6_slabs8", "k6_random5", "wave_xslabs4"]


def interface_points(grp):
    """The centroids of the group's new interface faces (face_index1 of a split
    without old communicators lists exactly those) and their sorted vertices."""
    f1 = grp["face_index1"].astype(np.int64)
    j, f = f1 // 12, (f1 % 12) // 3
    v = grp["tetra_v"][j[:, None], S.IDIR[f]]
    return grp["xyz"][v].mean(axis=1), np.sort(v, axis=1)


def step_points(grp, n):
    x, t = M.new_points(n)
    ix, fv = interface_points(grp)
    pts = np.concatenate([x, ix])
    tags = np.concatenate([t, np.full(len(ix), M.TAG_BDY, np.uint16)])
    return pts, tags, len(x), {tuple(r) for r in fv.tolist()}


def on_interface(mg, elem, faces):
    return sum(tuple(sorted(mg.tria[e].tolist())) in faces for e in elem)


def bare_mesh(d):
    """The fetched group as a mesh without trias and without Mmg's adjacency."""
    ne = d["tetra_v"].shape[0] - 1
    return M.Mesh(d["xyz"], d["tetra_v"], np.zeros(4 * ne + 5, np.int32), np.zeros((1, 3), np.int32),
                  np.zeros(4, np.int32))


def same_fetch(a, b):
    for k in S.INT_KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["xyz"][1:].tobytes() == b["xyz"][1:].tobytes()
    for x, y in zip(a["sols"], b["sols"]):
        assert x[1:].tobytes() == y[1:].tobytes()


def same_results(a, sa, b, sb):
    """elem and every solution byte equal.  status and steps equal wherever the
    two walks started from the same element (starts(), recorded), and most
    starts agree; where they differ, located or not is equal.  The hint build
    leaves a volume walk's start to a plain store (any sampled tet of the cell;
    pmx_starts.hip), and in a group that is not convex the start decides
    whether the walk or the exhaustive scan finds the tet, the sign of status:
    point 375 of group 1 of k6_random5 came out 1 (2 steps) or -1 (5 steps) in
    5 of 60 step pairs between two contexts that uploaded the same mesh.  The
    rule of tests/test_gpu_walk_store.py (assert_same, capped)."""
    same = sa == sb
    assert same.mean() > 0.5
    assert np.array_equal(a.elem, b.elem)
    for x, y in zip(a.sols, b.sols):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(a.status[same], b.status[same]) and np.array_equal(a.steps[same], b.steps[same])
    assert np.array_equal(a.status == 0, b.status == 0)
    return int(np.count_nonzero(~same)), int(np.count_nonzero(a.status != b.status))


def steps_equal(both, pts, tags):
    """A default and a FRESH step on both contexts: same_results between the
    contexts and between the two steps.  Returns the first context's default
    result and (points whose starts differed, points whose status differed),
    summed over the comparisons."""
    first = None
    ndiff = np.zeros(2, np.int64)
    for flags in (0, N.RUN_FRESH_BACKGROUND):
        res = []
        for t in both:
            t.upload_points(pts, tags)
            t.run(flags=flags, record_starts=True)
            res.append((t.download(), t.starts()))
        (a, sa), (b, sb) = res
        ndiff += same_results(a, sa, b, sb)
        if first is None:
            first = (a, sa)
        else:
            ndiff += same_results(a, sa, *first)
    return first[0], ndiff


# ---- 1. adopt equals upload -----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", CASES)
def test_adopt_equals_upload(transfer, name):
    m, part, ngrp, n = case(name)
    sols = sols_of(m)
    transfer.upload_background(m, sols, 0)
    transfer.split_groups(part, ngrp)
    adopted, uploaded = Transfer(0), Transfer(0)
    try:
        for g in range(ngrp):
            grp = transfer.split_fetch(g)
            mg = S.group_mesh(grp)
            transfer.split_adopt(g, adopted, imet=0, surface=True, hausd=mg.hausd)
            uploaded.upload_background(mg, grp["sols"], 0, adja=False)
            both = (adopted, uploaded)
            (ta, aa), (tb, ab) = (t.download_surface() for t in both)
            assert mg.nt > 0 and ta.shape == (mg.nt + 1, 3)
            assert ta.tobytes() == tb.tobytes() == mg.tria.tobytes()
            assert aa.tobytes() == ab.tobytes() == mg.adjt.tobytes()
            for w in (True, False):
                a, b = (t.metis_graph(weights=w) for t in both)
                for x, y in zip(a, b):
                    assert (x is None and y is None) or np.array_equal(x, y)
            a, b = (t.contiguity() for t in both)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert adopted.qualhisto() == uploaded.qualhisto()
            assert adopted.prilen() == uploaded.prilen()
            pts, tags, ncube, faces = step_points(grp, n)
            r, ndiff = steps_equal(both, pts, tags)
            print(name, g, "points whose starts / status differed:", ndiff.tolist(), "of", 3 * len(pts))
            # what the group contains is located: the CPU oracle on the same inputs says which
            # (every query fresh from the uploading context's start tria, as the parity tests run it)
            _, _, ostatus, *_ = Oracle(mg).interp(pts, tags, grp["sols"], fresh=True, start_bdy=uploaded.starts())
            assert np.all(ostatus[ncube:] != 0) and np.any(ostatus[:ncube] != 0)
            assert np.all(r.status[ostatus != 0] != 0)
            assert on_interface(mg, r.elem[ncube:], faces) > 0
            same_fetch(transfer.split_fetch(g), grp)          # the plan survives the adopt
    finally:
        adopted.close()
        uploaded.close()
        transfer.split_release()


# ---- 2. the plan survives -------------------------------------------------------------------

@gpu
def test_plan_survives_and_adopted_groups_split_again(transfer):
    m, part, ngrp, _ = case("k3_slabs3")
    transfer.upload_background(m, sols_of(m), 0)
    transfer.split_groups(part, ngrp)
    before = [transfer.split_fetch(g) for g in range(ngrp)]
    ctxs = [Transfer(0) for _ in range(ngrp)]
    other = Transfer(0)
    try:
        for g, t in enumerate(ctxs):
            transfer.split_adopt(g, t)
        for g in range(ngrp):
            same_fetch(transfer.split_fetch(g), before[g])
        # every adopted context holds its own group; a further split of it
        # equals the same split of the uploaded group
        for g, t in enumerate(ctxs):
            mg = S.group_mesh(before[g])
            other.upload_background(mg, before[g]["sols"], 0, adja=False)
            part2 = S.x_slabs(mg, 2)
            a, b = (c.split_groups(part2, 2) for c in (t, other))
            assert np.array_equal(a["sizes"], b["sizes"]) and np.array_equal(a["tet_new"], b["tet_new"])
            assert (a["int_face_nitem"], a["int_node_nitem"]) == (b["int_face_nitem"], b["int_node_nitem"])
            for h in range(2):
                same_fetch(t.split_fetch(h), other.split_fetch(h))
    finally:
        for t in ctxs + [other]:
            t.close()
        transfer.split_release()


# ---- 3. surface=False -----------------------------------------------------------------------

@gpu
def test_without_surface_equals_bare_upload(transfer):
    m, part, ngrp, n = case("k6_slabs6")
    transfer.upload_background(m, sols_of(m), 0)
    transfer.split_groups(part, ngrp)
    adopted, uploaded = Transfer(0), Transfer(0)
    try:
        grp = transfer.split_fetch(2)
        transfer.split_adopt(2, adopted, surface=False)
        uploaded.upload_background(bare_mesh(grp), grp["sols"], 0, adja=False)
        both = (adopted, uploaded)
        for t in both:
            tria, adjt = t.download_surface()
            assert tria.shape == (1, 3) and adjt.shape == (4,) and not adjt.any()
        a, b = (t.metis_graph() for t in both)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        x, tags = M.new_points(n, surface=False)              # no trias: a surface point would be refused
        r, _ = steps_equal(both, x, tags)
        assert np.any(r.status != 0)
    finally:
        adopted.close()
        uploaded.close()
        transfer.split_release()


# ---- 4. refusals ----------------------------------------------------------------------------

def raw_surface(tr, cap):
    tria = np.full((cap + 1, 3), SENT, np.int32)
    adjt = np.full(3 * cap + 4, SENT, np.int32)
    r = tr.lib.pmx_download_surface(tr.ctx, tria.ctypes.data_as(N.iptr), cap, adjt.ctypes.data_as(N.iptr))
    return r, tria, adjt, tr.lib.pmx_last_error(tr.ctx)


@gpu
def test_refusals_leave_dst_and_src_untouched(transfer):
    m, part, ngrp, n = case("k3_slabs3")
    transfer.upload_background(m, sols_of(m), 0)
    lib = transfer.lib
    dst = Transfer(0)
    try:
        # no background yet: nothing to download, sentinels intact
        r, tria, adjt, err = raw_surface(dst, 8)
        assert r == -1 and np.all(tria == SENT) and np.all(adjt == SENT) and b"no background" in err
        assert lib.pmx_download_surface(dst.ctx, None, 0, None) == -1          # the size query too
        # dst's previous background, and what a step on it gives
        m0 = M.kuhn_cube(2)
        s0 = [M.on_vertices(m0, M.iso_metric)]
        dst.upload_background(m0, s0, 0)
        x, tags = M.new_points(2)

        def step_bytes():
            dst.upload_points(x, tags)
            dst.run()
            r = dst.download()
            return b"".join([r.elem.tobytes(), r.status.tobytes()] + [a.tobytes() for a in r.sols])

        ref_bytes = step_bytes()
        # the uploaded trias come back, and too small an array is refused
        tria, adjt = dst.download_surface()
        assert tria.tobytes() == m0.tria.tobytes() and adjt.tobytes() == m0.adjt.tobytes()
        assert lib.pmx_download_surface(dst.ctx, None, 0, None) == m0.nt        # tria NULL: nt alone
        r, tria, adjt, err = raw_surface(dst, m0.nt - 1)
        assert r == -1 and np.all(tria == SENT) and np.all(adjt == SENT) and b"maxnt" in err
        r, tria, adjt, err = raw_surface(dst, m0.nt + 3)
        assert r == m0.nt and np.all(tria[0] == SENT) and np.all(tria[m0.nt + 1:] == SENT)
        assert np.array_equal(tria[1:m0.nt + 1], m0.tria[1:])

        def refused(what, src, g, d, imet=0, surface=1, hausd=0.01):
            r = lib.pmx_split_adopt(src, g, d, imet, surface, hausd)
            err = lib.pmx_last_error(d)
            assert r == 0 and what in err, err
            assert dst.kernel_ms(ADOPT_SLOT) == -1.0
            assert step_bytes() == ref_bytes                  # dst keeps its background

        refused(b"no plan", transfer.ctx, 0, dst.ctx)
        transfer.split_groups(part, ngrp)
        before = [transfer.split_fetch(g) for g in range(ngrp)]
        refused(b"src is NULL", None, 0, dst.ctx)
        assert lib.pmx_split_adopt(transfer.ctx, 0, None, 0, 1, 0.01) == 0
        assert b"dst is NULL" in lib.pmx_last_error(None)
        assert lib.pmx_split_adopt(transfer.ctx, 0, transfer.ctx, 0, 1, 0.01) == 0
        assert b"dst is src" in lib.pmx_last_error(transfer.ctx)
        refused(b"group out of range", transfer.ctx, -1, dst.ctx)
        refused(b"group out of range", transfer.ctx, ngrp, dst.ctx)
        refused(b"imet", transfer.ctx, 0, dst.ctx, imet=-2)
        refused(b"imet", transfer.ctx, 0, dst.ctx, imet=2)
        refused(b"surface must be 0 or 1", transfer.ctx, 0, dst.ctx, surface=2)
        refused(b"surface must be 0 or 1", transfer.ctx, 0, dst.ctx, surface=-1)
        for h in (-1.0, float("nan"), float("inf")):
            refused(b"hausd", transfer.ctx, 0, dst.ctx, hausd=h)
        for g in range(ngrp):
            same_fetch(transfer.split_fetch(g), before[g])    # src still fetches
        # and the context takes a good adopt right after
        transfer.split_adopt(1, dst)
        assert dst.kernel_ms(ADOPT_SLOT) > 0.0
        assert dst.download_surface()[0].tobytes() == S.group_mesh(before[1]).tria.tobytes()
    finally:
        dst.close()
        transfer.split_release()


@gpu
def test_adopt_refuses_non_manifold_faces():
    """Three tets on one face: the adopt fails as the upload does, dst holds no
    background, src still fetches."""
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [1, 1, -1],
                    [2, 0, 0], [2, 1, 0], [2, 0, 1], [3, 0, 0]], np.float64)
    tv = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [1, 3, 2, 5], [1, 3, 2, 6], [7, 8, 9, 10]], np.int32)
    adja = np.zeros(4 * 4 + 5, np.int32)                      # Mmg's adjacency as given: no neighbour anywhere
    mesh = M.Mesh(xyz, tv, adja, np.zeros((1, 3), np.int32), np.zeros(4, np.int32))
    src, dst = Transfer(0), Transfer(0)
    try:
        src.upload_background(mesh, [np.ones((11, 1))], 0)
        src.split_groups(np.array([0, 0, 0, 1], np.int32), 2)
        grp = src.split_fetch(0)
        m0 = M.kuhn_cube(2)
        dst.upload_background(m0, [np.ones((m0.np + 1, 1))], 0)
        for surface in (True, False):
            with pytest.raises(RuntimeError, match="non-manifold"):
                src.split_adopt(0, dst, surface=surface)
            with pytest.raises(RuntimeError):
                dst.metis_graph(weights=False)                # no background
            assert dst.kernel_ms(ADOPT_SLOT) == -1.0
        assert np.array_equal(src.split_fetch(0)["tetra_v"], grp["tetra_v"])
        src.split_adopt(1, dst)                               # the other group is fine
        assert dst.download_surface()[0].shape == (5, 3)
    finally:
        src.close()
        dst.close()


# ---- 5. the oracle meets the conditions (CPU) -----------------------------------------------

def test_oracle_locates_interface_centroids_on_interface_trias():
    """Pins the inputs of test_adopt_equals_upload: on the 6-slab case the CPU
    oracle locates every interface-centroid point of every group, and on a
    tria of an interface face.  Passes without the feature."""
    m, part, ngrp, n = case("k6_slabs6")
    sp = S.split(m, part, ngrp, data=(m.xyz, sols_of(m)))
    for grp in sp["groups"]:
        mg = S.group_mesh(grp)
        pts, tags, ncube, faces = step_points(grp, n)
        assert mg.nt > 0 and len(pts) > ncube
        _, elem, status, *_ = Oracle(mg).interp(pts, tags, grp["sols"])
        assert np.all(status[ncube:] != 0) and np.any(status[:ncube] != 0)
        assert on_interface(mg, elem[ncube:], faces) > 0


# ---- 6. lifecycle and timing ----------------------------------------------------------------

@gpu
def test_adopt_leaves_nothing_behind_and_times_itself():
    m, part, ngrp, _ = case("k3_slabs3")
    sols = sols_of(m)
    lib = N.load()
    before = lib.pmx_debug_live_allocations()
    src, dst = Transfer(0), Transfer(0)
    try:
        assert dst.kernel_ms(ADOPT_SLOT) == -1.0 and src.kernel_ms(ADOPT_SLOT) == -1.0
        src.upload_background(m, sols, 0)
        src.split_groups(part, ngrp)
        src.split_adopt(0, dst)
        assert dst.kernel_ms(ADOPT_SLOT) > 0.0 and src.kernel_ms(ADOPT_SLOT) == -1.0
        assert lib.pmx_debug_live_allocations() > before
        src.split_adopt(1, dst, surface=False)
        src.split_release()
        dst.download_surface()
    finally:
        src.close()
        dst.close()
    assert lib.pmx_debug_live_allocations() == before
