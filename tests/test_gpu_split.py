"""pmx_split_groups / pmx_split_fetch on the GPU against the CPU twin
(tests/c/split_ref.c): the new groups of PMMG_split_eachGrp (reference
src/grpsplit_pmmg.c:1267-1445).

Everything is compared for equality: sizes, tet_new, both final nitem, the
eight integer arrays of every group, and the xyz and solution rows bit for bit
(they are copies).  No tolerance appears anywhere.

Two of the refusals of pmx_split_groups (4*ne >= 2^31 and 12*ne_g + 11 >= 2^31)
need a group of more than 178 M tets and are not exercised here."""
import ctypes as C

import numpy as np
import pytest

import split_ref as S
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

SENT = -77
PLAN_SLOT, FETCH_SLOT = 14, 15


def sols_of(m):
    return [M.on_vertices(m, M.iso_metric), M.on_vertices(m, M.velocity)]


def upload(tr, m, adja=True, sols=None):
    sols = sols if sols is not None else [np.ones((m.np + 1, 1))]
    tr.upload_background(m, sols, 0, adja=adja)
    return sols


def same_group(got, ref, data=True):
    for k in S.INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    if data:
        assert got["xyz"][1:].tobytes() == ref["xyz"][1:].tobytes()
        assert len(got["sols"]) == len(ref["sols"])
        for a, b in zip(got["sols"], ref["sols"]):
            assert a[1:].tobytes() == b[1:].tobytes()


def check_split(tr, m, part, ngrp, comm=None, sols=None, groups=None, ref=None):
    """The device's split equals the twin's; returns (plan dict, twin dict)."""
    ref = ref if ref is not None else S.split(m, part, ngrp, comm, data=(m.xyz, sols) if sols is not None else None)
    got = tr.split_groups(part, ngrp, comm)
    assert np.array_equal(got["sizes"], ref["sizes"])
    assert got["tet_new"].dtype == np.int32 and np.array_equal(got["tet_new"], ref["tet_new"])
    assert got["int_face_nitem"] == ref["int_face_nitem"] and got["int_node_nitem"] == ref["int_node_nitem"]
    for g in (range(ngrp) if groups is None else groups):
        same_group(tr.split_fetch(g, data=sols is not None), ref["groups"][g], data=sols is not None)
    return got, ref


# ---- 1. basics ---------------------------------------------------------------------------

@pytest.mark.parametrize("ngrp", [2, 3])
def test_slabs_with_metric_and_field(transfer, ngrp):
    m = M.kuhn_cube(3)
    sols = upload(transfer, m, sols=sols_of(m))
    check_split(transfer, m, S.slabs(m, ngrp), ngrp, sols=sols)
    assert transfer.kernel_ms(PLAN_SLOT) > 0.0 and transfer.kernel_ms(FETCH_SLOT) > 0.0


# ---- 2. numbering variants ---------------------------------------------------------------

@pytest.mark.parametrize("variant", ["adja", "device_adja", "shuffle"])
def test_eight_slabs_numberings(transfer, variant):
    m = M.kuhn_cube(6)
    part = S.slabs(m, 8)
    if variant == "shuffle":
        # the same mesh renumbered is a different problem (the orders go by
        # tet number), so the twin runs again on it
        m, tinv = M.numbering(m, "shuffle")
        p = np.zeros(m.ne, np.int32)
        p[tinv[1:] - 1] = part
        part = p
    sols = upload(transfer, m, adja=variant != "device_adja", sols=sols_of(m))
    check_split(transfer, m, part, 8, sols=sols)


# ---- 3. winding and random interfaces ----------------------------------------------------

def test_boustrophedon_and_random(transfer):
    m = M.kuhn_cube(6)
    sols = upload(transfer, m)
    check_split(transfer, m, S.boustrophedon(m, 6), 2, sols=sols)
    part = S.fix_empty(np.random.default_rng(7).integers(0, 5, m.ne), 5)
    check_split(transfer, m, part, 5, sols=sols)


# ---- 4. many groups ----------------------------------------------------------------------

def test_thousand_groups(transfer):
    m = M.kuhn_cube(6)
    sols = upload(transfer, m)
    check_split(transfer, m, S.modulo_parts(m.ne, 1000), 1000, sols=sols)


# ---- 5. an unstructured mesh -------------------------------------------------------------

def test_wave_mesh(transfer):
    m = S.wave_mesh()
    sols = upload(transfer, m, sols=sols_of(m))
    check_split(transfer, m, S.x_slabs(m, 4), 4, sols=sols)


# ---- 6. non-manifold, old communicators --------------------------------------------------

@pytest.mark.parametrize("ids", [(0, 2, 1), (1, 2, 0)])
def test_non_manifold(transfer, ids):
    m, ne_a, corner = S.glued_cubes()
    sols = upload(transfer, m)
    got, ref = check_split(transfer, m, S.glued_parts(m, ne_a, ids), 3, sols=sols)
    gb = transfer.split_fetch(ids[2], data=False)
    lp = int(np.nonzero(gb["point_old"] == corner)[0][0]) + 1
    assert (lp in gb["node_index1"].tolist()) == (ids[2] == 1)


def test_old_communicators_pass_through(transfer):
    m = M.kuhn_cube(4)
    sols = upload(transfer, m)
    got, ref = check_split(transfer, m, S.slabs(m, 2), 2, sols=sols)
    g0 = transfer.split_fetch(0)
    m0 = S.group_mesh(g0)
    x = m0.centroids()[:, 0]
    part2 = (x >= np.median(x)).astype(np.int32)
    comm = S.group_comm(g0, got)
    sols0 = upload(transfer, m0)
    got2, ref2 = check_split(transfer, m0, part2, 2, comm, sols=sols0)
    assert got2["int_face_nitem"] > got["int_face_nitem"] and got2["int_node_nitem"] > got["int_node_nitem"]
    # duplicated input entries: the last one wins, as in the reference's loops
    dup = dict(comm)
    dup["face_index1"] = np.concatenate([comm["face_index1"], comm["face_index1"][:3]])
    dup["face_index2"] = np.concatenate([comm["face_index2"], comm["face_index2"][:3] + 1000])
    dup["node_index1"] = np.concatenate([comm["node_index1"], comm["node_index1"][:3]])
    dup["node_index2"] = np.concatenate([comm["node_index2"], comm["node_index2"][:3] + 1000])
    check_split(transfer, m0, part2, 2, dup, sols=sols0)


# ---- 7. independent of the twin ----------------------------------------------------------

@pytest.mark.parametrize("nslab", [8, 6])
def test_against_device_topology(transfer, nslab):
    """The device face matching, the labelling and the Metis graph on every new
    group.  6 slabs follow the cell layers of the n = 6 cube, so each is one
    component; 8 slabs (case 2's partition) are thinner than a cell and fall
    into pieces -- as many as the part has in the old mesh (pmx_contiguity on
    the old group, and the breadth-first twin of the contiguity tests)."""
    import contiguity_ref as R
    m = M.kuhn_cube(6)
    part = S.slabs(m, nslab)
    upload(transfer, m)
    _, counts, _ = transfer.contiguity(part, nslab)
    assert np.array_equal(counts, R.components(m, part, nslab)[1])
    if nslab == 6:
        assert np.all(counts == 1)
    plan = transfer.split_groups(part, nslab)
    groups = [transfer.split_fetch(g) for g in range(nslab)]
    for g, grp in enumerate(groups):
        npg = int(plan["sizes"][g][1])
        assert np.array_equal(transfer.build_adja(grp["tetra_v"], npg), grp["adja"])
    for g, grp in enumerate(groups):
        mg = S.group_mesh(grp)
        upload(transfer, mg)
        ncomp, _, _ = transfer.contiguity()
        assert ncomp == counts[g]
        xadj, _, _ = transfer.metis_graph(weights=False)
        assert xadj[-1] == np.count_nonzero(grp["adja"])


# ---- 8. determinism ----------------------------------------------------------------------

def test_determinism(transfer):
    m = M.kuhn_cube(6)
    sols = upload(transfer, m, sols=sols_of(m))
    part = S.fix_empty(np.random.default_rng(7).integers(0, 5, m.ne), 5)

    def run(order):
        plan = transfer.split_groups(part, 5)
        out = {g: transfer.split_fetch(g) for g in order}
        blob = [plan["sizes"].tobytes(), plan["tet_new"].tobytes()]
        for g in range(5):
            blob += [out[g][k].tobytes() for k in S.INT_KEYS] + [out[g]["xyz"].tobytes()]
            blob += [a.tobytes() for a in out[g]["sols"]]
        return b"".join(blob), plan["int_face_nitem"], plan["int_node_nitem"]

    assert run(range(5)) == run(range(5)) == run(range(4, -1, -1))


# ---- 9. refusals -------------------------------------------------------------------------

def raw_plan(tr, part, ngrp, ne, comm=None, null_part=False):
    sizes = (N.SplitSizes * max(ngrp, 1))()
    for s in sizes:
        s.ne = s.np = s.nface = s.nnode = SENT
    tet_new = np.full(ne, SENT, np.int32)
    fn, nn = C.c_int64(SENT), C.c_int64(SENT)
    c = None
    keep = []
    if comm is not None:
        c = N.SplitComm()
        for k in ("face_index1", "face_index2", "node_index1", "node_index2"):
            a = np.ascontiguousarray(comm.get(k, np.zeros(0)), np.int32)
            keep.append(a)
            setattr(c, k, a.ctypes.data_as(N.iptr) if a.size else None)
        c.nface, c.nnode = len(keep[0]), len(keep[2])
        c = C.byref(c)
    r = tr.lib.pmx_split_groups(tr.ctx, None if null_part else part.ctypes.data_as(N.i32ptr), ngrp, c, sizes,
                                tet_new.ctypes.data_as(N.iptr), C.byref(fn), C.byref(nn))
    clean = (all(s.ne == SENT and s.np == SENT and s.nface == SENT and s.nnode == SENT for s in sizes)
             and np.all(tet_new == SENT) and fn.value == SENT and nn.value == SENT)
    return r, clean, tr.lib.pmx_last_error(tr.ctx)


def raw_fetch(tr, g, n=64):
    arr = {k: np.full(n, SENT, np.int32) for k in S.INT_KEYS}
    xyz = np.full(n, float(SENT))
    o = N.SplitOut()
    for k, a in arr.items():
        setattr(o, k, a.ctypes.data_as(N.iptr))
    o.xyz = xyz.ctypes.data_as(N.dptr)
    r = tr.lib.pmx_split_fetch(tr.ctx, g, C.byref(o))
    clean = all(np.all(a == SENT) for a in arr.values()) and np.all(xyz == SENT)
    return r, clean, tr.lib.pmx_last_error(tr.ctx)


def test_refusals_leave_outputs_untouched(transfer):
    m = M.kuhn_cube(3)
    part = np.ascontiguousarray(S.slabs(m, 3))
    ne = m.ne
    tr = Transfer(0)
    try:
        r, clean, err = raw_plan(tr, part, 3, ne)
        assert r == 0 and clean and b"upload a group first" in err
        r, clean, err = raw_fetch(tr, 0)
        assert r == 0 and clean and b"no plan" in err
        assert tr.kernel_ms(PLAN_SLOT) == -1.0 and tr.kernel_ms(FETCH_SLOT) == -1.0
    finally:
        tr.close()
    upload(transfer, m)
    r, clean, err = raw_fetch(transfer, 0)
    assert r == 0 and clean and b"no plan" in err

    def refused(what, *a, **kw):
        r, clean, err = raw_plan(transfer, *a, **kw)
        assert r == 0 and clean and what in err, err
        # and a fetch finds no plan after a refused call
        r, clean, err = raw_fetch(transfer, 0)
        assert r == 0 and clean and b"no plan" in err

    refused(b"part is NULL", part, 3, ne, null_part=True)
    refused(b"ngrp < 1", part, 0, ne)
    bad = part.copy()
    bad[5] = 3
    refused(b"outside 0..ngrp-1", bad, 3, ne)
    bad[5] = -1
    refused(b"outside 0..ngrp-1", bad, 3, ne)
    refused(b"empty", part, 4, ne)                          # part 3 has no tet
    refused(b"empty", np.where(part == 1, 2, part).astype(np.int32), 3, ne)
    refused(b"empty", part, ne + 1, ne)
    f_ok = S.split(m, part, 3)["groups"][0]
    bdy = np.nonzero(m.adja[1:4 * ne + 1] == 0)[0]          # boundary faces: 4*(k-1) + f
    inner = np.nonzero(m.adja[1:4 * ne + 1] != 0)[0]
    enc = lambda i: np.array([12 * (i // 4 + 1) + 3 * (i % 4)], np.int32)
    one = np.array([0], np.int32)
    refused(b"outside 12..12*ne+11", part, 3, ne, comm={"face_index1": np.array([11], np.int32), "face_index2": one})
    refused(b"outside 12..12*ne+11", part, 3, ne,
            comm={"face_index1": np.array([12 * ne + 12], np.int32), "face_index2": one})
    refused(b"adjacency is not 0", part, 3, ne, comm={"face_index1": enc(inner[0]), "face_index2": one})
    refused(b"outside 1..np", part, 3, ne, comm={"node_index1": np.array([0], np.int32), "node_index2": one})
    refused(b"outside 1..np", part, 3, ne, comm={"node_index1": np.array([m.np + 1], np.int32), "node_index2": one})
    # a deleted tet: the reference wants a packed mesh
    md = M.Mesh(m.xyz, m.tet.copy(), m.adja, m.tria, m.adjt)
    md.tet[77, 0] = 0
    upload(transfer, md)
    refused(b"deleted tet", part, 3, ne)
    with pytest.raises(RuntimeError, match="deleted tet"):
        transfer.split_groups(part, 3)
    # the context is usable: a correct call right after succeeds
    upload(transfer, m)
    r, clean, err = raw_plan(transfer, part, 3, ne, comm={"face_index1": enc(bdy[0]), "face_index2": one})
    assert r == 1 and not clean
    check_split(transfer, m, part, 3)
    # g out of range
    for g in (-1, 3):
        r, clean, err = raw_fetch(transfer, g)
        assert r == 0 and clean and b"out of range" in err
    r, clean, err = raw_fetch(transfer, 0, n=4 * int(f_ok["tetra_v"].size) + 64)
    assert r == 1 and not clean
    # solution views that do not match the uploaded ones
    with pytest.raises(RuntimeError, match="solution"):
        saved, transfer.sizes = transfer.sizes, [3]
        try:
            transfer.split_fetch(0)
        finally:
            transfer.sizes = saved
    # a new background drops the plan; so does a release
    upload(transfer, m)
    r, clean, err = raw_fetch(transfer, 0)
    assert r == 0 and clean and b"no plan" in err
    with pytest.raises(RuntimeError, match="no plan"):
        transfer.split_fetch(0)
    check_split(transfer, m, part, 3)
    transfer.split_release()
    r, clean, err = raw_fetch(transfer, 0)
    assert r == 0 and clean and b"no plan" in err
    assert transfer.kernel_ms(PLAN_SLOT) == -1.0
    check_split(transfer, m, part, 3)


def test_promoted_background_drops_the_plan(transfer):
    m1, m2 = M.kuhn_cube(3, seed=101), M.kuhn_cube(4)
    x2 = m2.xyz[1:].copy()
    onb = np.any((x2 == 0.0) | (x2 == 1.0), axis=1)
    t2 = np.where(onb, M.TAG_BDY, 0).astype(np.uint16)
    tets2 = m2.tet.copy() - 1
    tets2[0] = -1
    tr = Transfer(0)
    try:
        upload(tr, m1)
        tr.split_groups(S.slabs(m1, 2), 2)
        tr.upload_points(x2, t2, tets2)
        tr.run()
        r2 = tr.download()
        tr.split_fetch(0)                                   # a step leaves the plan alone
        tr.promote_background(m2, r2.sols, adja=False)
        with pytest.raises(RuntimeError, match="no plan"):
            tr.split_fetch(0)
        # the promoted group splits as a fresh upload of the same mesh would
        sols2 = [np.concatenate([np.zeros((1, a.shape[1])), a]) for a in r2.sols]
        check_split(tr, m2, S.slabs(m2, 3), 3, sols=sols2)
    finally:
        tr.close()


# ---- 10. timers --------------------------------------------------------------------------

def test_timers():
    tr = Transfer(0)
    try:
        assert tr.kernel_ms(PLAN_SLOT) == -1.0 and tr.kernel_ms(FETCH_SLOT) == -1.0
        m = M.kuhn_cube(3)
        upload(tr, m)
        tr.split_groups(S.slabs(m, 2), 2)
        assert tr.kernel_ms(PLAN_SLOT) > 0.0 and tr.kernel_ms(FETCH_SLOT) == -1.0
        tr.split_fetch(1)
        assert tr.kernel_ms(FETCH_SLOT) > 0.0
    finally:
        tr.close()
