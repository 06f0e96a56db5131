"""pmx_merge_groups_from on the GPU: a merge whose groups lie in contexts on the
device (the two merges of PMMG_split_n2mGrps, reference
src/loadbalancing_pmmg.c:88,135), a held group possibly with unused points and
deleted tets (the skips of PMMG_merge_grps, src/mergemesh_pmmg.c:346,507,710).

Every comparison is for equality; no tolerance appears anywhere.  The
yardstick is the CPU twin of the merge (merge_ref.merge) on host arrays; for
groups that are not packed, the twin on the groups packed with numpy, with
tet_old, point_old and the maps composed back (merge_from_ref.expected)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_from_ref as U
import merge_ref as R
import moveifc_ref as F
import split_ref as S
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = R.SENT
PLAN_SLOT, FETCH_SLOT, ADOPT_SLOT = 16, 17, 18
CASES = {k: v for k, v in R.cases().items() if v[2] <= 8}


def case_groups(name):
    if name == "k6_slabs3":          # more than one 256-thread block of row elements and of tets per group
        m = M.kuhn_cube(6)
        sp, comm = R.split_case(m, S.slabs(m, 3), 3, R.sols_of(m))
    elif name == "k1_one":           # 6 tets: under one wave
        m = M.kuhn_cube(1)
        return [{"tetra_v": m.tet, "xyz": m.xyz, "sols": R.sols_of(m)}], None
    else:
        m, part, ngrp, sols = CASES[name]
        sp, comm = R.split_case(m, part, ngrp, sols)
    return sp["groups"], comm


def bare_mesh(d):
    """A group as a mesh without trias and without Mmg's adjacency."""
    ne = d["tetra_v"].shape[0] - 1
    return M.Mesh(np.ascontiguousarray(d["xyz"]), np.ascontiguousarray(d["tetra_v"], np.int32),
                  np.zeros(4 * ne + 5, np.int32), np.zeros((1, 3), np.int32), np.zeros(4, np.int32))


def hold(grp):
    """A context of its own that uploaded the group, with its solutions.  The
    upload without Mmg's adjacency takes deleted tets (rows with v[0] <= 0)."""
    tr = Transfer(0)
    tr.upload_background(bare_mesh(grp), grp["sols"], 0, adja=False)
    return tr


def entries(grp):
    return {k: grp[k] for k in U.IDX if k in grp}


def held_source(tr, grp):
    return dict(entries(grp), held=tr)


def close_all(trs):
    for t in trs:
        if t is not None:
            t.close()


def same_fetch(got, ref):
    for k in R.INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    assert got["xyz"][1:].tobytes() == ref["xyz"][1:].tobytes()
    assert len(got["sols"]) == len(ref["sols"])
    for a, b in zip(got["sols"], ref["sols"]):
        assert a[1:].tobytes() == b[1:].tobytes()


def check_from(tr, sources, ref):
    """merge_groups_from equals ref: sizes, every fetched array, both maps of every group."""
    got = tr.merge_groups_from(sources, ref["comm"])
    assert np.array_equal(got["sizes"], ref["sizes"])
    same_fetch(tr.merge_fetch(), ref)
    for g in range(len(sources)):
        pn, tn = tr.merge_maps(g)
        assert pn.dtype == np.int32 and np.array_equal(pn, ref["maps"][g][0]), g
        assert tn.dtype == np.int32 and np.array_equal(tn, ref["maps"][g][1]), g


def blob(tr, ngrp):
    d = tr.merge_fetch()
    out = [d[k].tobytes() for k in R.INT_KEYS] + [d["xyz"][1:].tobytes()] + [a[1:].tobytes() for a in d["sols"]]
    for g in range(ngrp):
        out += [a.tobytes() for a in tr.merge_maps(g)]
    return b"".join(out)


# ---- 1. held equals host --------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES) + ["k6_slabs3", "k1_one"])
def test_held_equals_host(transfer, name):
    groups, comm = case_groups(name)
    ref = dict(R.merge(groups, comm), comm=comm)
    holders = [hold(g) for g in groups]
    try:
        check_from(transfer, [held_source(t, g) for t, g in zip(holders, groups)], ref)
        assert transfer.kernel_ms(PLAN_SLOT) > 0.0 and transfer.kernel_ms(FETCH_SLOT) > 0.0
    finally:
        close_all(holders)
        transfer.merge_release()


# ---- 2. host and held sources in one call ---------------------------------------------------

def remote():
    m = M.kuhn_cube(6)
    part = S.fix_empty(np.random.default_rng(11).integers(0, 3, m.ne), 3)
    _, groups, comm, _ = R.remote_case(m, part, 2, R.sols_of(m))
    return groups, comm


def duplicate():
    m = M.kuhn_cube(3)
    _, groups, comm, _ = R.remote_case(m, S.slabs(m, 3), 1)
    g0, g1 = dict(groups[0]), dict(groups[1])
    free_n, free_f = comm["int_node_nitem"], comm["int_face_nitem"]
    comm = dict(comm, int_node_nitem=free_n + 2, int_face_nitem=free_f + 1)
    cat = lambda a, b: np.concatenate([a, b]).astype(np.int32)
    g0["node_index1"], g0["node_index2"] = cat(g0["node_index1"], [1, 2]), cat(g0["node_index2"], [free_n, free_n])
    g0["face_index1"], g0["face_index2"] = cat(g0["face_index1"], [12, 27]), cat(g0["face_index2"], [free_f, free_f])
    g1["node_index1"] = cat(g1["node_index1"], g1["node_index1"][:1])
    g1["node_index2"] = cat(g1["node_index2"], [free_n + 1])
    comm["ext_node"] = [cat(comm["ext_node"][0], [free_n])]
    comm["ext_face"] = [cat(comm["ext_face"][0], [free_f])]
    return [g0, g1], comm


@pytest.mark.parametrize("make", [remote, duplicate])
@pytest.mark.parametrize("held0", [True, False])
def test_mixed_sources_equal_all_host(transfer, make, held0):
    groups, comm = make()
    transfer.merge_groups(groups, comm)
    host = blob(transfer, len(groups))
    host_sizes = transfer._merge["sizes"].copy()
    ref = dict(R.merge(groups, comm), comm=comm)
    holders = [hold(g) if (i == 0) == held0 else None for i, g in enumerate(groups)]
    try:
        src = [held_source(t, g) if t is not None else g for t, g in zip(holders, groups)]
        check_from(transfer, src, ref)
        assert np.array_equal(transfer._merge["sizes"], host_sizes) and blob(transfer, len(groups)) == host
        check_from(transfer, groups, ref)                 # and every source from the host, through this entry
        assert blob(transfer, len(groups)) == host
    finally:
        close_all(holders)
        transfer.merge_release()


# ---- 3. every kind of holder ----------------------------------------------------------------

def test_split_adopted_and_merge_adopted_holders(transfer):
    """Groups made resident by split_adopt, then the merged group -- resident
    in `transfer` by merge_adopt -- as the only source of a merge into
    `transfer` itself: each gives the bytes of the uploaded holder."""
    m, part, ngrp, sols = CASES["k3_slabs3"]
    groups, comm = case_groups("k3_slabs3")
    ref = dict(R.merge(groups, comm), comm=comm)
    src, holders = Transfer(0), [Transfer(0) for _ in groups]
    try:
        src.upload_background(m, sols, 0)
        src.split_groups(part, ngrp)
        for g, t in enumerate(holders):
            src.split_adopt(g, t, 0, surface=bool(g % 2))
        check_from(transfer, [held_source(t, g) for t, g in zip(holders, groups)], ref)
        merged = transfer.merge_fetch()
        transfer.merge_adopt(0)
        one = {"tetra_v": merged["tetra_v"], "xyz": merged["xyz"], "sols": merged["sols"]}
        ref1 = dict(R.merge([one]), comm=None)
        check_from(transfer, [{"held": transfer}], ref1)        # ctx is its own source
        assert np.array_equal(transfer.merge_fetch()["tetra_v"], merged["tetra_v"])
        up = hold(one)
        holders.append(up)
        transfer.merge_groups_from([{"held": up}])
        a = blob(transfer, 1)
        transfer.merge_groups_from([{"held": transfer}])
        assert blob(transfer, 1) == a
        # the same context twice: two copies of the group, no shared entries
        two = dict(R.merge([one, one]), comm=None)
        check_from(transfer, [{"held": up}, {"held": up}], two)
    finally:
        close_all([src] + holders)
        transfer.merge_release()


def test_promoted_holder():
    """A group promoted after a step (the setup of tests/test_gpu_resident.py):
    its vertices are the step's new points, its solutions the step's results."""
    m1 = M.kuhn_cube(5, seed=101)
    sols1 = [M.on_vertices(m1, M.iso_metric), M.on_vertices(m1, M.velocity)]
    m2 = M.kuhn_cube(6, seed=202)
    x = m2.xyz[1:].copy()
    onb = np.any((x == 0.0) | (x == 1.0), axis=1)
    tets0 = m2.tet.copy() - 1
    tets0[0] = -1
    tr, up, dst = Transfer(0), Transfer(0), Transfer(0)
    try:
        tr.upload_background(m1, sols1, 0)
        tr.upload_points(x, np.where(onb, M.TAG_BDY, 0).astype(np.uint16), tets0)
        tr.run()
        r = tr.download(init=[np.full((len(x), s.shape[1]), -3.0) for s in sols1])
        tr.promote_background(m2, r.sols)
        rows = [np.concatenate([np.zeros((1, s.shape[1])), s]) for s in r.sols]
        grp = {"tetra_v": m2.tet, "xyz": m2.xyz, "sols": rows}
        ref = dict(R.merge([grp]), comm=None)
        check_from(dst, [{"held": tr}], ref)
        a = blob(dst, 1)
        up.upload_background(m2, rows, 0)
        check_from(dst, [{"held": up}], ref)
        assert blob(dst, 1) == a
    finally:
        close_all([tr, up, dst])


# ---- 4. groups that are not packed ----------------------------------------------------------

def unpacked_case():
    """kuhn_cube(8) in two slabs (405 points, 1536 tets each), both groups with
    unused points at id 1, at id np and in a run across 256, and deleted tets
    first, last and in a run across 256 and across 1024."""
    m = M.kuhn_cube(8)
    sp, comm = R.split_case(m, S.slabs(m, 2), 2, R.sols_of(m))
    out = []
    for g, grp in enumerate(sp["groups"]):
        npk, nek = grp["xyz"].shape[0] - 1, grp["tetra_v"].shape[0] - 1
        ph = [1] + list(range(250 + g, 262 + g))
        ph.append(npk + len(ph) + 1)
        th = [1] + list(range(253 - g, 259)) + list(range(1020, 1030))
        th.append(nek + len(th) + 1)
        out.append(U.unpack_group(grp, np.array(ph), np.array(th)))
    return out, comm


def test_unpacked_groups(transfer):
    groups, comm = unpacked_case()
    ref = dict(U.expected(groups, comm), comm=comm)
    for g, grp in enumerate(groups):                      # group 0 and a group >= 1 drop points and tets
        pn, tn = ref["maps"][g]
        assert (pn == 0).sum() >= 14 and (tn == 0).sum() >= 14
        assert pn[0] == 0 and pn[-1] == 0 and tn[0] == 0 and tn[-1] == 0 and np.any(pn[254:258] == 0)
        assert grp["tetra_v"][1, 0] <= 0 and grp["tetra_v"][-1, 0] <= 0
    holders = [hold(g) for g in groups]
    other = None
    try:
        check_from(transfer, [held_source(t, g) for t, g in zip(holders, groups)], ref)
        # group 0 held and not packed, group 1 from the host, packed
        packed1 = U.pack_group(groups[1])[0]
        mixed = dict(U.expected([groups[0], packed1], comm), comm=comm)
        check_from(transfer, [held_source(holders[0], groups[0]), packed1], mixed)
        check_from(transfer, [held_source(t, g) for t, g in zip(holders, groups)], ref)
        transfer.merge_adopt(0)
        d = transfer.merge_fetch()
        other = Transfer(0)
        other.upload_background(bare_mesh(d), d["sols"], 0, adja=False)
        for w in (True, False):
            a, b = (t.metis_graph(weights=w) for t in (transfer, other))
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(x, y)
        part = S.x_slabs(bare_mesh(d), 3)
        a, b = (t.contiguity(part, 3) for t in (transfer, other))
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    finally:
        close_all(holders + [other])
        transfer.merge_release()


# ---- 5. refusals ----------------------------------------------------------------------------

def raw_from(tr, sources, comm, edit=None):
    gv, ns, c, meta, keep = tr._merge_views(sources, comm)
    sv = (N.MergeSource * len(sources))()
    for g, d in enumerate(sources):
        sv[g].held = d["held"].ctx if d.get("held") is not None else None
        sv[g].g = gv[g]
    if edit is not None:
        edit(sv)
    sz = N.MergeSizes(SENT, SENT, SENT, SENT)
    r = tr.lib.pmx_merge_groups_from(tr.ctx, len(sources), sv, ns, C.byref(c), C.byref(sz))
    return r, (sz.np, sz.ne, sz.nnode, sz.nface) == (SENT,) * 4, tr.lib.pmx_last_error(tr.ctx)


def raw_fetch(tr, n=64):
    arr = {k: np.full(n, SENT, np.int32) for k in R.INT_KEYS}
    o = N.MergeOut()
    for k, a in arr.items():
        setattr(o, k, a.ctypes.data_as(N.iptr))
    r = tr.lib.pmx_merge_fetch(tr.ctx, C.byref(o))
    return r, all(np.all(a == SENT) for a in arr.values()), tr.lib.pmx_last_error(tr.ctx)


def test_refusals_leave_everything_untouched(transfer):
    """Every refused call names `cont`, a holder of the packed group 1, beside
    the unpacked holder of group 0 (in either order): afterwards `cont` answers
    contiguity and the Metis graph with its former results, and both holders
    still give the good merge.

    A held tet with a vertex out of range is not exercised: every install
    path (upload, promotion, the adopts) refuses or cannot produce such a
    background, so no holder can be brought into that state through the API."""
    groups, comm = unpacked_case()
    packed = [U.pack_group(g)[0] for g in groups]
    ref = ref_mixed(groups, packed, comm)
    h0, cont = hold(groups[0]), hold(packed[1])
    one_sol, other_size, empty = Transfer(0), Transfer(0), Transfer(0)
    try:
        p1 = packed[1]
        one_sol.upload_background(bare_mesh(p1), p1["sols"][:1], 0, adja=False)
        other_size.upload_background(bare_mesh(p1), [p1["sols"][0], p1["sols"][0]], 0, adja=False)
        part1 = S.x_slabs(bare_mesh(p1), 2)
        src0, src1 = held_source(h0, groups[0]), held_source(cont, p1)
        good = [src0, src1]
        former = cont.contiguity(part1, 2)
        former_graph = cont.metis_graph(weights=False)

        def refused(what, sources, c=None, edit=None):
            assert not sources or any(d.get("held") is cont for d in sources)
            transfer.merge_groups_from(good, comm)        # a good plan first: the refused call leaves none
            r, clean, err = raw_from(transfer, sources, c if c is not None else comm, edit)
            assert r == 0 and clean and what in err, err
            assert transfer.kernel_ms(PLAN_SLOT) == -1.0
            r, clean, err = raw_fetch(transfer)
            assert r == 0 and clean and b"no plan" in err

        def edited(base, key, at, value):
            d = dict(base)
            a = np.array(d[key], np.int32)
            a[at] = value
            d[key] = a
            return d

        np0, ne0 = groups[0]["xyz"].shape[0] - 1, groups[0]["tetra_v"].shape[0] - 1
        np1, ne1 = p1["xyz"].shape[0] - 1, p1["tetra_v"].shape[0] - 1
        # entries on dropped entities of the unpacked holder, as group 0 and as group 1
        refused(b"names a dropped point", [edited(src0, "node_index1", 0, np0), src1])
        refused(b"names a dropped point: no valid tet holds it (group 1)", [src1, edited(src0, "node_index1", 0, 1)])
        refused(b"names a dropped tet", [edited(src0, "face_index1", 0, 12 * ne0 + 3), src1])
        refused(b"names a dropped tet (v[0] <= 0) (group 1)", [src1, edited(src0, "face_index1", -1, 12 * 255)])
        # the holders' own state
        refused(b"no background", [src1, dict(entries(p1), held=empty)])
        refused(b"nsol differs", [src1, dict(entries(p1), held=one_sol)])
        refused(b"solution sizes differ", [src1, dict(entries(p1), held=other_size)])
        # the entries of the packed holder itself
        refused(b"point outside 1..np", [src0, edited(src1, "node_index1", 0, np1 + 1)])
        refused(b"outside 12..12*ne+11", [src0, edited(src1, "face_index1", 0, 12 * ne1 + 12)])
        refused(b"position outside 0..int_node_nitem-1", [src0, edited(src1, "node_index2", 0, comm["int_node_nitem"])])
        refused(b"NULL view", good, edit=lambda sv: setattr(sv[1].g, "node_index2", None))
        # the refusals of host sources, through this entry, the holder beside them
        host0 = U.pack_group(groups[0])[0]
        tv = host0["tetra_v"].copy()
        tv[5, 0] = 0
        refused(b"deleted tet", [dict(host0, tetra_v=tv), src1])
        tv = host0["tetra_v"].copy()
        tv[5, 2] = host0["xyz"].shape[0]
        refused(b"vertex outside 1..np", [src1, dict(host0, tetra_v=tv)])
        refused(b"sizes differ", [src1, dict(host0, sols=[host0["sols"][0], host0["sols"][0]])])
        refused(b"point outside 1..np", [src1, edited(host0, "node_index1", 0, 0)])
        refused(b"NULL view", [src1, host0], edit=lambda sv: setattr(sv[1].g, "point_c", None))
        refused(b"ngrp < 1", [])
        # the holders the refused calls named are as they were
        again = cont.contiguity(part1, 2)
        assert again[0] == former[0] and np.array_equal(again[1], former[1]) and np.array_equal(again[2], former[2])
        for x, y in zip(cont.metis_graph(weights=False), former_graph):
            assert (x is None and y is None) or np.array_equal(x, y)
        check_from(transfer, good, ref)
    finally:
        close_all([h0, cont, one_sol, other_size, empty])
        transfer.merge_release()


def ref_mixed(groups, packed, comm):
    return dict(U.expected([groups[0], packed[1]], comm), comm=comm)


# ---- 6. determinism and lifetime ------------------------------------------------------------

def test_two_calls_identical_bytes_and_holders_destroyed():
    groups, comm = unpacked_case()
    ref = dict(U.expected(groups, comm), comm=comm)
    lib = N.load()
    before = lib.pmx_debug_live_allocations()
    dst = Transfer(0)
    holders = [hold(g) for g in groups]
    try:
        src = [held_source(t, g) for t, g in zip(holders, groups)]
        dst.merge_groups_from(src, comm)
        a = blob(dst, 2)
        dst.merge_groups_from(src, comm)
        assert blob(dst, 2) == a
        close_all(holders)                                # right after the call
        holders = []
        same_fetch(dst.merge_fetch(), ref)
        dst.merge_adopt(0)
        d = dst.merge_fetch()
        same_fetch(d, ref)
        chk = hold({"tetra_v": d["tetra_v"], "xyz": d["xyz"], "sols": d["sols"]})
        holders.append(chk)
        for x, y in zip(dst.metis_graph(weights=False), chk.metis_graph(weights=False)):
            assert (x is None and y is None) or np.array_equal(x, y)
        assert lib.pmx_debug_live_allocations() > before
        dst.merge_release()
    finally:
        close_all(holders + [dst])
    assert lib.pmx_debug_live_allocations() == before
    # a refused call and a plan that its context's destruction frees
    for refuse in (True, False):
        dst, h = Transfer(0), hold(groups[0])
        try:
            if refuse:
                with pytest.raises(RuntimeError, match="no background"):
                    dst.merge_groups_from([{"held": dst}])
            else:
                dst.merge_groups_from([held_source(h, dict(groups[0], node_index1=[], node_index2=[], face_index1=[],
                                                           face_index2=[]))])
        finally:
            close_all([dst, h])
        assert lib.pmx_debug_live_allocations() == before


# ---- 7. through the chain -------------------------------------------------------------------

def test_chain_to_the_split(transfer):
    """held -> merge_adopt -> moveifc_begin(None) -> one layer -> moveifc_fix ->
    part_from_marks -> split_groups_part equals the chain from the all-host merge."""
    m = M.kuhn_cube(6)
    sp, comm = R.split_case(m, S.slabs(m, 4), 4)
    groups = sp["groups"]
    mp = F.single_map([g["tetra_v"].shape[0] - 1 for g in groups])

    def chain(tr):
        tr.merge_adopt(0)
        nfront = tr.moveifc_begin(None, mp)
        st = tr.moveifc_layer()
        tr.moveifc_fix()
        ngrp, gm = tr.part_from_marks(N.GRPSPL_MMG_TARGET)
        return nfront, st["recolor"], ngrp, tr.split_groups_part()

    holders = [hold(g) for g in groups]
    other = Transfer(0)
    try:
        transfer.merge_groups_from([held_source(t, g) for t, g in zip(holders, groups)], comm)
        a = chain(transfer)
        other.merge_groups(groups, comm)
        b = chain(other)
        assert a[:3] == b[:3] and a[0] > 0 and a[1] > 0
        assert np.array_equal(a[3]["sizes"], b[3]["sizes"]) and np.array_equal(a[3]["tet_new"], b[3]["tet_new"])
    finally:
        close_all(holders + [other])
        transfer.merge_release()


# ---- 8. the C driver ------------------------------------------------------------------------

DEMO_SRC = os.path.join(ROOT, "tests", "c", "merge_from_demo.c")
DEMO_BIN = os.path.join(ROOT, "tests", "c", "_build", "merge_from_demo")


def fnv(a) -> int:
    h = 1469598103934665603
    for x in np.asarray(a, np.int32).ravel().view(np.uint32).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_driver():
    os.makedirs(os.path.dirname(DEMO_BIN), exist_ok=True)
    gen = os.path.join(ROOT, "parmmg_amd", "csrc", "meshgen.c")
    deps = [DEMO_SRC, gen, os.path.join(ROOT, "include", "pmx_transfer.h"), N.LIB_PATH]
    if not os.path.exists(DEMO_BIN) or any(os.path.getmtime(DEMO_BIN) < os.path.getmtime(d) for d in deps):
        subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-std=c99", "-I",
                        os.path.join(ROOT, "include"), DEMO_SRC, gen, "-o", DEMO_BIN, "-L",
                        os.path.dirname(N.LIB_PATH), "-lpmx_transfer", "-Wl,-rpath," + os.path.dirname(N.LIB_PATH),
                        "-lm"], check=True)
    r = subprocess.run([DEMO_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "merge_from ok" in r.stdout, r.stdout + r.stderr
    m = M.kuhn_cube(6)
    part = (2 * np.arange(m.ne) // m.ne).astype(np.int32)
    met = (1.0 + 0.001 * np.arange(m.np + 1))[:, None]
    sp, comm = R.split_case(m, part, 2, [met])
    ref = R.merge(sp["groups"], comm)
    want = (f"merge_from np={m.np} ne={m.ne} nnode={ref['sizes'][2]} nface={ref['sizes'][3]} "
            f"tetra={fnv(ref['tetra_v'][1:]):016x} tet_old={fnv(ref['tet_old']):016x} "
            f"point_old={fnv(ref['point_old']):016x}")
    assert want in r.stdout, r.stdout
