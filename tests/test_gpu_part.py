"""pmx_part_* and pmx_split_groups_part on the GPU: the partition stays on the
device from the displacement's marks (or the host's Metis array) to the split.

pmx_part_from_marks is PMMG_part_getInterfaces (reference
src/moveinterfaces_pmmg.c:1150-1212) and is compared byte for byte with the
CPU twin's mir_part (tests/c/moveifc_ref.c) on the marks the twins of the
displacement, the fix and the reachability check leave; pmx_part_fix with the
contiguity twin; pmx_split_groups_part with pmx_split_groups of the downloaded
array on a second context and with the split twin.  No tolerance appears
anywhere.  The twins' runs are computed once per case and shared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contiguity_ref as R
import merge_ref as G
import moveifc_ref as F
import reach_ref as X
import split_ref as S
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77
PART_SLOT = 24
DISTR, MMG = N.GRPSPL_DISTR_TARGET, N.GRPSPL_MMG_TARGET
TWIN_FIELDS = ("ncomp", "nmerged", "nmerged_tets", "ncannot", "counter")


def lds_threshold() -> int:
    """The colour-table size up to which the kernels keep the table in LDS."""
    with open(os.path.join(ROOT, "parmmg_amd", "csrc", "pmx_part.hip"), encoding="utf-8") as fh:
        return int(re.search(r"^#define PT_LDS_COLOURS (\d+)", fh.read(), re.M).group(1))


def upload(tr, m):
    tr.upload_background(m, [np.ones((m.np + 1, 1))], 0)


@pytest.fixture
def second():
    tr = Transfer(0)
    yield tr
    tr.close()


# ---- the chains: the device and the twins side by side, up to the reachability check ---------------

_twins = {}


def twin_ranks3(name):
    """(m, tg, mp, node, nlayers, twin after its layers, marks after fix and check, entries, ngrps)."""
    if name not in _twins:
        m, tg, mp, node, begin, layers, t0 = F.run(name)
        t = F.Twin(m, tg, mp)
        for li in range(len(layers)):
            t.set_colors(node[0], F.exchange_fn(t.weight, node, li)(t.colors(node[0])))
            assert t.layer()[0]
        fi, rank = X.entries(m, 1 / 6)
        colors = (t.nprocs * np.arange(t.nold) + t.myrank).astype(np.int32)
        w = X.Twin(m, t.mark.copy())
        fixed, fst = w.fix(colors)
        c = fixed[fi // 12 - 1]
        cin = np.where(c % t.nprocs == rank, c, X.UNSET).astype(np.int32)
        ok, out, st = w.reach(fi, cin)
        assert ok
        out.setflags(write=False)
        _twins[name] = (m, tg, mp, node, len(layers), t, out, fi, rank, np.diff(mp["displsgrp"]).astype(np.int32))
    return _twins[name]


def device_ranks3(tr, name):
    """The device's chain of case `name` up to moveifc_reach; the twin's tuple."""
    d = twin_ranks3(name)
    m, tg, mp, node, nl, t, out, fi, rank, ngrps = d
    upload(tr, m)
    tr.moveifc_begin(tg, mp)
    for li in range(nl):
        tr.moveifc_set_colors(node[0], F.exchange_fn(t.weight, node, li)(tr.moveifc_colors(node[0])))
        tr.moveifc_layer()
    tr.moveifc_fix()
    sent = tr.reach_face_marks(None, fi)
    tr.moveifc_reach(fi, np.where(sent % t.nprocs == rank, sent, X.UNSET).astype(np.int32))
    assert tr.moveifc_marks().tobytes() == out.tobytes()
    return d


def twin_one_rank():
    if "one" not in _twins:
        m = M.kuhn_cube(6)
        x, y, z = R.cells(m, 6).T
        part = ((x >= 4) + 2 * (y >= 3)).astype(np.int32)
        sp, comm = G.split_case(m, part, 4)
        groups = sp["groups"]
        twin_merge = G.merge(groups, comm)
        mm = M.from_tets(twin_merge["xyz"], twin_merge["tetra_v"])
        mp = F.single_map([g["tetra_v"].shape[0] - 1 for g in groups])
        t = F.Twin(mm, twin_merge["tet_group"], mp)
        for _ in range(2):
            assert t.layer()[0]
        fi, rank = X.entries(mm, 1 / 6)
        w = X.Twin(mm, t.mark.copy())
        fixed, fst = w.fix(np.arange(4, dtype=np.int32))
        ok, out, st = w.reach(fi, np.full(len(fi), X.UNSET, np.int32))
        assert ok
        out.setflags(write=False)
        _twins["one"] = (groups, comm, mm, mp, t, out, fi)
    return _twins["one"]


def device_one_rank(tr):
    d = twin_one_rank()
    groups, comm, mm, mp, t, out, fi = d
    tr.merge_groups(groups, comm)
    tr.merge_adopt(0)
    tr.moveifc_begin(None, mp)
    for _ in range(2):
        tr.moveifc_layer()
    tr.moveifc_fix()
    tr.moveifc_reach(fi, np.full(len(fi), X.UNSET, np.int32))
    assert tr.moveifc_marks().tobytes() == out.tobytes()
    return d


def mesh_comm(m, node_points):
    """Old communicators of the whole mesh for the split: the boundary faces of
    the bottom and top layers and the listed points, numbered from 100 on."""
    fi, _ = X.entries(m, 1 / 6)
    pts = np.ascontiguousarray(node_points, np.int32)
    return {"face_index1": fi, "face_index2": (100 + np.arange(len(fi))).astype(np.int32),
            "node_index1": pts, "node_index2": (100 + np.arange(len(pts))).astype(np.int32),
            "int_face_nitem": 100 + len(fi), "int_node_nitem": 100 + len(pts)}


def same_plan(got, ref):
    assert np.array_equal(got["sizes"], ref["sizes"])
    assert got["tet_new"].dtype == np.int32 and np.array_equal(got["tet_new"], ref["tet_new"])
    assert got["int_face_nitem"] == ref["int_face_nitem"] and got["int_node_nitem"] == ref["int_node_nitem"]


def check_split_part(tr, other, m, comm, upload_other=None):
    """3.: split_groups_part on tr equals split_groups(downloaded part) on
    `other` (the same background) and the split twin, every array of every group."""
    part, ngrp = tr.part_download()
    got = tr.split_groups_part(comm)
    (upload_other or upload)(other, m)
    ref = other.split_groups(part, ngrp, comm)
    twin = S.split(m, part, ngrp, comm)
    same_plan(got, ref)
    same_plan(got, twin)
    for g in range(ngrp):
        a, b = tr.split_fetch(g), other.split_fetch(g)
        for k in S.INT_KEYS:
            assert a[k].dtype == np.int32 and np.array_equal(a[k], b[k]) and np.array_equal(a[k], twin["groups"][g][k]), k
        assert a["xyz"][1:].tobytes() == b["xyz"][1:].tobytes()
        for u, v in zip(a["sols"], b["sols"]):
            assert u[1:].tobytes() == v[1:].tobytes()


def check_group_mark(part, ngrp, gm, marks):
    assert gm.dtype == np.int32 and len(gm) == ngrp
    for g in range(ngrp):
        u = np.unique(marks[part == g])
        assert len(u) == 1 and u[0] == gm[g], g


# ---- 1. + 3. DISTR target, three ranks ---------------------------------------------------------------

# sizes: the twin's groups on the marks after the fix and the check (on the marks
# right after the layers ranks3 gives 6 / 426 / 216 / 586 / 62); no part is empty
@pytest.mark.parametrize("name,sizes", [("ranks3", [5, 432, 219, 586, 54]), ("ranks3_big", [134, 576, 586])])
@pytest.mark.parametrize("with_comm", [True, False])
def test_distr_three_ranks(transfer, second, name, sizes, with_comm):
    m, tg, mp, node, nl, t, out, fi, rank, ngrps = device_ranks3(transfer, name)
    ok, tp, tn = t.part(DISTR, ngrps, mark=out)
    assert ok and np.bincount(tp, minlength=tn).tolist() == sizes
    ngrp, gm = transfer.part_from_marks(DISTR, ngrps)
    assert transfer.kernel_ms(PART_SLOT) > 0.0
    part, n2 = transfer.part_download()
    assert ngrp == n2 == tn and part.dtype == np.int32 and part.tobytes() == tp.tobytes()
    check_group_mark(part, ngrp, gm, out)
    # the owners PMMG_part_getProcs reads: ranks3 ends with marks of all three ranks
    assert set(gm % 3) == set(out % 3) and (name != "ranks3" or len(set(gm % 3)) == 3)
    # ngrps_all = NULL is the map's
    n3, gm3 = transfer.part_from_marks(DISTR)
    assert n3 == ngrp and np.array_equal(gm3, gm) and transfer.part_download()[0].tobytes() == tp.tobytes()
    transfer.moveifc_release()
    check_split_part(transfer, second, m, mesh_comm(m, node[0]) if with_comm else None)


# ---- 2. + 3. MMG target, one rank ----------------------------------------------------------------------

@pytest.mark.parametrize("with_comm", [True, False])
def test_mmg_one_rank(transfer, second, with_comm):
    groups, comm, mm, mp, t, out, fi = device_one_rank(transfer)
    ok, tp, tn = t.part(MMG, mark=out)
    assert ok and tn == 4 and np.bincount(tp, minlength=4).tolist() == [216, 468, 216, 396]
    ngrp, gm = transfer.part_from_marks(MMG)
    part, n2 = transfer.part_download()
    assert ngrp == n2 == 4 and part.tobytes() == tp.tobytes()
    assert np.array_equal(gm, t.nprocs * np.arange(4) + t.myrank)
    check_group_mark(part, ngrp, gm, out)
    transfer.moveifc_release()
    pts = (np.nonzero(mm.xyz[1:, 0] == 0.0)[0] + 1).astype(np.int32)
    check_split_part(transfer, second, mm, mesh_comm(mm, pts) if with_comm else None)


# ---- 4. upload, fix, split: the Metis path ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["random_6_3_1", "random_4_5_2", "cascade6"])
def test_upload_fix_split(transfer, second, name):
    m, part, col, fpart, st = R.case(name)
    assert np.ndim(col) == 0                                        # the split form: colours 0..n-1
    upload(transfer, m)
    transfer.part_upload(part, int(col))
    got, ngrp = transfer.part_download()
    assert ngrp == col and got.tobytes() == np.asarray(part, np.int32).tobytes()
    gst = transfer.part_fix()
    assert {k: gst[k] for k in TWIN_FIELDS} == st
    assert transfer.kernel_ms(12) > 0.0
    got, ngrp = transfer.part_download()
    assert ngrp == col and got.tobytes() == fpart.tobytes()
    # the host call gives the same array and the same stats, the launch counts included
    upload(second, m)
    host_part, hst = second.fix_contiguity(part, col)
    assert host_part.tobytes() == got.tobytes() and hst == gst
    assert np.bincount(fpart, minlength=int(col)).min() > 0         # no part is empty: the split accepts it
    check_split_part(transfer, second, m, None)


# ---- 5. tails and alignment ------------------------------------------------------------------------------

def first_tets(n):
    """The first n tets of a Kuhn cube as a mesh of their own points."""
    k = M.kuhn_cube(2)
    tet = k.tet[:n + 1].copy()
    used = np.unique(tet[1:])
    new = np.zeros(k.np + 1, np.int32)
    new[used] = np.arange(1, len(used) + 1)
    tet[1:] = new[tet[1:]]
    return M.from_tets(np.concatenate([[[0.0, 0.0, 0.0]], k.xyz[used]]), tet)


@pytest.mark.parametrize("ne", [1, 2, 3, 4, 5, 6, 7, 8, 9, "cube1"])
def test_tails_and_alignment(transfer, ne):
    m = M.kuhn_cube(1) if ne == "cube1" else first_tets(ne)
    tg = (np.arange(m.ne) % 3).astype(np.int32)
    tg[0] = 2
    displs = np.array([0, 1, 4, 6], np.int32)
    mp = {"nprocs": 3, "myrank": 1, "displsgrp": displs, "mapgrp": np.array([5, 7, 7, 7, 3, 4], np.int32)}
    t = F.Twin(m, tg, mp)
    upload(transfer, m)
    transfer.moveifc_begin(tg, mp)
    assert transfer.moveifc_marks().tobytes() == t.mark.tobytes()
    for target, ngrps in [(MMG, None), (DISTR, None), (DISTR, np.array([2, 3, 1], np.int32))]:
        ok, tp, tn = t.part(target, ngrps)
        assert ok
        ngrp, gm = transfer.part_from_marks(target, ngrps)
        part, n2 = transfer.part_download()
        assert ngrp == n2 == tn and part.tobytes() == tp.tobytes(), (target, ngrps)
        if target == DISTR:
            check_group_mark(part, ngrp, gm, t.mark)
        # the host call through the same kernels
        p2, n3 = transfer.moveifc_part(None, target, ngrps)
        assert n3 == tn and p2.tobytes() == tp.tobytes()


# ---- 6. a table larger than the LDS path -------------------------------------------------------------------

def test_table_past_the_lds_threshold(transfer):
    m, tg, mp, node, nl, t, out, fi, rank, ngrps = device_ranks3(transfer, "ranks3")
    thr = lds_threshold()
    results = []
    for ng in (np.array([1, thr + 5, 2], np.int32), np.array([1, thr - 3, 2], np.int32), ngrps):
        assert (int(ng.sum()) > thr) == (ng[1] == thr + 5)
        ok, tp, tn = t.part(DISTR, ng, mark=out)
        assert ok
        ngrp, gm = transfer.part_from_marks(DISTR, ng)
        part, _ = transfer.part_download()
        assert ngrp == tn and part.tobytes() == tp.tobytes()
        check_group_mark(part, ngrp, gm, out)
        results.append(part.tobytes())
    # the numbering goes by rank and group, not by the table's size
    assert results[0] == results[1] == results[2]


# ---- 7. determinism and the timer ----------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_the_timer():
    tr = Transfer(0)
    try:
        assert tr.kernel_ms(PART_SLOT) == -1.0
        m, tg, mp, node, nl, t, out, fi, rank, ngrps = device_ranks3(tr, "ranks3_big")
        assert tr.kernel_ms(PART_SLOT) == -1.0
        runs = []
        for _ in range(2):
            ngrp, gm = tr.part_from_marks(DISTR, ngrps)
            assert tr.kernel_ms(PART_SLOT) > 0.0
            runs.append((ngrp, gm.tobytes(), tr.part_download()[0].tobytes()))
        assert runs[0] == runs[1]
        assert tr.lib.pmx_part_from_marks(tr.ctx, 7, None, None, None) == 0          # a refusal
        assert tr.kernel_ms(PART_SLOT) == -1.0
        tr.part_from_marks(DISTR, ngrps)
        assert tr.kernel_ms(PART_SLOT) > 0.0
        upload(tr, m)
        assert tr.kernel_ms(PART_SLOT) == -1.0
    finally:
        tr.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------

def raw_from_marks(tr, target, ngrps_all):
    n = C.c_int32(SENT)
    gm = np.full(64, SENT, np.int32)
    ng = None if ngrps_all is None else np.ascontiguousarray(ngrps_all, np.int32)
    r = tr.lib.pmx_part_from_marks(tr.ctx, target, ng.ctypes.data_as(N.iptr) if ng is not None else None, C.byref(n),
                                   gm.ctypes.data_as(N.i32ptr))
    return r, n.value == SENT and bool(np.all(gm == SENT)), tr.lib.pmx_last_error(tr.ctx)


def raw_without_partition(tr, ne):
    """split_groups_part, part_fix and part_download are refused, outputs untouched."""
    lib, ctx = tr.lib, tr.ctx
    part = np.full(max(ne, 1), SENT, np.int32)
    n = C.c_int32(SENT)
    assert lib.pmx_part_download(ctx, part.ctypes.data_as(N.i32ptr), C.byref(n)) == 0
    assert b"no partition" in lib.pmx_last_error(ctx) and n.value == SENT and np.all(part == SENT)
    st = N.ContigStats()
    st.counter = SENT
    assert lib.pmx_part_fix(ctx, 0, C.byref(st)) == 0 and st.counter == SENT
    assert b"no partition" in lib.pmx_last_error(ctx)
    sizes = (N.SplitSizes * 8)()
    sizes[0].ne = SENT
    tn = np.full(max(ne, 1), SENT, np.int32)
    fn, nn = C.c_int64(SENT), C.c_int64(SENT)
    assert lib.pmx_split_groups_part(ctx, None, sizes, tn.ctypes.data_as(N.iptr), C.byref(fn), C.byref(nn)) == 0
    assert sizes[0].ne == SENT and np.all(tn == SENT) and fn.value == SENT and nn.value == SENT
    return lib.pmx_last_error(ctx)


def test_refusals_leave_outputs_and_the_partition(transfer):
    tr = Transfer(0)
    try:
        r, clean, err = raw_from_marks(tr, DISTR, None)                       # no group uploaded
        assert r == 0 and clean and err
        assert tr.lib.pmx_part_upload(tr.ctx, np.zeros(4, np.int32).ctypes.data_as(N.i32ptr), 1) == 0
        assert b"upload a group first" in tr.lib.pmx_last_error(tr.ctx)
        assert b"upload a group first" in raw_without_partition(tr, 4)
    finally:
        tr.close()

    m, tg, mp, node, nl, t, out, fi, rank, ngrps = twin_ranks3("ranks3")
    upload(transfer, m)
    assert b"no partition" in raw_without_partition(transfer, m.ne)
    r, clean, err = raw_from_marks(transfer, DISTR, ngrps)                    # no live displacement
    assert r == 0 and clean and b"pmx_moveifc_begin" in err

    device_ranks3(transfer, "ranks3")
    assert set(np.unique(out)) >= {0, 1, 4, 7}
    held = (np.arange(m.ne) % 3).astype(np.int32)
    transfer.part_upload(held, 3)

    def still_held():
        part, ngrp = transfer.part_download()
        return ngrp == 3 and part.tobytes() == held.tobytes()

    for what, target, ng, word in [
        ("an unknown target", 0, ngrps, b"unknown target"),
        ("an unknown target", 3, ngrps, b"unknown target"),
        ("MMG with a foreign mark", MMG, None, b"another rank"),
        ("ngrps_all < 0", DISTR, [1, -1, 2], b"ngrps_all < 0"),
        ("a mark of no group", DISTR, [1, 2, 2], b"a mark of no group"),
        ("a mark of no group", DISTR, [0, 3, 2], b"a mark of no group"),
    ]:
        r, clean, err = raw_from_marks(transfer, target, ng)
        assert r == 0 and clean and word in err, what
        assert transfer.kernel_ms(PART_SLOT) == -1.0 and still_held(), what
    # the refusal names the same tet on every call
    errs = {raw_from_marks(transfer, DISTR, [1, 2, 2])[2] for _ in range(3)}
    first = int(np.nonzero(out == 7)[0][0]) + 1
    assert len(errs) == 1 and f"tet {first} ".encode() in errs.pop()

    lib, ctx = transfer.lib, transfer.ctx
    for bad, ngrp, word in [(held, 0, b"ngrp < 1"), (held, 2, b"outside 0..ngrp-1"),
                            (np.where(np.arange(m.ne) == 5, -1, held).astype(np.int32), 3, b"outside 0..ngrp-1")]:
        assert lib.pmx_part_upload(ctx, bad.ctypes.data_as(N.i32ptr), ngrp) == 0
        assert word in lib.pmx_last_error(ctx) and still_held()
    assert lib.pmx_part_upload(ctx, None, 3) == 0 and still_held()
    st = N.ContigStats()
    st.counter = SENT
    assert lib.pmx_part_fix(ctx, -1, C.byref(st)) == 0 and st.counter == SENT and still_held()

    # an empty part: one group too many
    transfer.part_upload(held, 4)
    sizes = (N.SplitSizes * 4)()
    sizes[0].ne = SENT
    tn = np.full(m.ne, SENT, np.int32)
    fn, nn = C.c_int64(SENT), C.c_int64(SENT)
    assert lib.pmx_split_groups_part(ctx, None, sizes, tn.ctypes.data_as(N.iptr), C.byref(fn), C.byref(nn)) == 0
    assert b"part 3 is empty" in lib.pmx_last_error(ctx)
    assert sizes[0].ne == SENT and np.all(tn == SENT) and fn.value == SENT and nn.value == SENT
    part, ngrp = transfer.part_download()
    assert ngrp == 4 and part.tobytes() == held.tobytes()
    with pytest.raises(RuntimeError):
        transfer.split_fetch(0)
    # pmx_split_groups without an array is still "part is NULL"
    assert lib.pmx_split_groups(ctx, None, 3, None, sizes, None, None, None) == 0
    assert b"part is NULL" in lib.pmx_last_error(ctx)
    # after all that the calls still work
    ngrp, gm = transfer.part_from_marks(DISTR, ngrps)
    assert transfer.part_download()[0].tobytes() == t.part(DISTR, ngrps, mark=out)[1].tobytes()
    transfer.part_release()
    assert b"no partition" in raw_without_partition(transfer, m.ne)


# ---- 9. lifecycle -----------------------------------------------------------------------------------------------

def test_lifecycle(transfer, second):
    m, tg, mp, node, nl, t, out, fi, rank, ngrps = device_ranks3(transfer, "ranks3")
    ok, tp, tn = t.part(DISTR, ngrps, mark=out)
    transfer.part_from_marks(DISTR, ngrps)
    # the host call in between leaves the held partition alone
    p, n = transfer.moveifc_part(None, DISTR, np.array([2, 3, 2], np.int32))
    tw = t.part(DISTR, np.array([2, 3, 2], np.int32), mark=out)
    assert tw[0] and p.tobytes() == tw[1].tobytes() and n == tw[2]
    assert transfer.part_download()[0].tobytes() == tp.tobytes()
    # ... and survives the release of the displacement
    transfer.moveifc_release()
    part, ngrp = transfer.part_download()
    assert ngrp == tn and part.tobytes() == tp.tobytes()
    assert transfer.lib.pmx_part_from_marks(transfer.ctx, DISTR, None, None, None) == 0
    assert transfer.part_download()[0].tobytes() == tp.tobytes()

    # split_adopt into a context drops that context's partition, not the giver's
    upload(second, m)
    second.part_upload(tp, tn)
    transfer.split_groups_part()
    transfer.split_adopt(0, second)
    assert b"no partition" in raw_without_partition(second, m.ne)
    assert transfer.part_download()[0].tobytes() == tp.tobytes()
    # upload_background
    upload(transfer, m)
    assert b"no partition" in raw_without_partition(transfer, m.ne)
    # merge_adopt
    groups, comm, mm, mp1, t1, out1, fi1 = twin_one_rank()
    transfer.part_upload(tp, tn)
    transfer.merge_groups(groups, comm)
    assert transfer.part_download()[1] == tn                        # the plan alone does not
    transfer.merge_adopt(0)
    assert b"no partition" in raw_without_partition(transfer, mm.ne)


# ---- 10. the C driver ---------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(ROOT, "tests", "c", "part_demo.c")
DEMO_BIN = os.path.join(ROOT, "tests", "c", "_build", "part_demo")


def build_demo() -> str:
    os.makedirs(os.path.dirname(DEMO_BIN), exist_ok=True)
    gen = os.path.join(ROOT, "parmmg_amd", "csrc", "meshgen.c")
    deps = [DEMO_SRC, gen, os.path.join(ROOT, "include", "pmx_transfer.h"), N.LIB_PATH]
    if (not os.path.exists(DEMO_BIN)
            or any(os.path.getmtime(DEMO_BIN) < os.path.getmtime(d) for d in deps if os.path.exists(d))):
        subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-std=c99", "-I",
                        os.path.join(ROOT, "include"), DEMO_SRC, gen, "-o", DEMO_BIN, "-L",
                        os.path.dirname(N.LIB_PATH), "-lpmx_transfer",
                        "-Wl,-rpath," + os.path.dirname(N.LIB_PATH), "-lm"], check=True)
    return DEMO_BIN


def test_c_driver(transfer):
    r = subprocess.run([build_demo()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "part ok" in r.stdout
