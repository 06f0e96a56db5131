"""pmx_moveifc_* on the GPU against the CPU twin (tests/c/moveifc_ref.c):
PMMG_set_color_tetra, PMMG_mark_interfacePoints, the layers of
PMMG_part_moveInterfaces and PMMG_part_getInterfaces (reference
src/moveinterfaces_pmmg.c:119-134, 832-1090, 1150-1212, 1306-1440).

Everything is compared for equality after begin and after every layer: the
marks, tmp, s, the front, negrp and every stats field the twin has.  The
twin's runs are computed once per case (moveifc_ref.run) and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contiguity_ref as R
import merge_ref as G
import moveifc_ref as F
import split_ref as S
from conftest import ROOT
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

SENT = -77
BEGIN_SLOT, LAYER_SLOT = 19, 20
TWIN_STATS = ("front", "touched", "recolor", "next", "blocks", "maxball", "blocked")


def upload(tr, m, adja=True):
    tr.upload_background(m, [np.ones((m.np + 1, 1))], 0, adja=adja)


def state(tr):
    tmp, s, front = tr.moveifc_points()
    negrp, nemin = tr.moveifc_groups()
    return {"mark": tr.moveifc_marks(), "tmp": tmp, "s": s, "front": front, "negrp": negrp, "nemin": nemin}


def same_state(tr, snap, what=""):
    got = state(tr)
    for k in ("mark", "tmp", "s", "front", "negrp", "nemin"):
        assert np.array_equal(got[k], snap[k]), (what, k, int((got[k] != snap[k]).sum()))
    return got


def check_case(tr, name, adja=True, seq_steps=0):
    """begin and every layer of a case equal the twin's; returns the layers' stats."""
    m, tg, mp, node, begin, layers, t = F.run(name)
    upload(tr, m, adja)
    assert tr.moveifc_begin(tg, mp) == begin["nfront"]
    same_state(tr, begin, "begin")
    out = []
    for li, (ok, st, snap) in enumerate(layers):
        assert ok
        if node is not None:
            pts = node[0]
            tr.moveifc_set_colors(pts, F.exchange_fn(t.weight, node, li)(tr.moveifc_colors(pts)))
            assert tr.moveifc_points()[2][pts - 1].all()          # every listed point is front
        got = tr.moveifc_layer(seq_steps)
        print(name, li, got)
        assert {k: got[k] for k in TWIN_STATS} == {k: st[k] for k in TWIN_STATS}, (name, li)
        same_state(tr, snap, f"layer {li}")
        out.append(got)
    return out


# ---- 1. empty fronts --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["empty_slabs", "equal_slabs"])
def test_empty_front(transfer, name):
    st = check_case(transfer, name)
    assert F.run(name)[4]["nfront"] == 0 and all(s["front"] == 0 and s["recolor"] == 0 for s in st)


# ---- 2. - 4. the parallel path -----------------------------------------------------------------

@pytest.mark.parametrize("adja", [True, False], ids=["adja", "device_adja"])
@pytest.mark.parametrize("name", F.PARALLEL_CASES + F.SHUFFLED_PARALLEL)
def test_parallel_path(transfer, name, adja):
    st = check_case(transfer, name, adja)
    clean = [s["blocked"] == 0 for s in st]
    if name.startswith("octants"):
        assert clean == [True, True, False]
    else:
        assert all(clean)                                        # the parallel path is what was compared
    if name == "revquad":
        assert [s["front"] for s in st] == [49, 97, 97] and all(s["recolor"] == 216 for s in st)
    if name == "ties":
        assert st[3]["next"] == 0


def test_two_runs_give_identical_bytes(transfer):
    m, tg, mp, node, begin, layers, t = F.run("frag_6_big")
    runs = []
    for _ in range(2):
        upload(transfer, m)
        transfer.moveifc_begin(tg, mp)
        per = [state(transfer)]
        for _ in layers:
            transfer.moveifc_layer()
            per.append(state(transfer))
        runs.append(per)
    for a, b in zip(*runs):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- 4. - 6. the sequential path ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["frag_4_counts", "frag_6_counts", "revslabs", "tiny"] + F.SHUFFLED_BLOCKING)
def test_blocking_layers(transfer, name):
    st = check_case(transfer, name)
    blocked = [s["blocked"] for s in st]
    if name.startswith("frag_6_counts"):
        assert blocked[:2] == [1, 1]
    if name == "revslabs":
        assert blocked == [0, 1] and st[1]["blocks"] == 3
    assert any(blocked) and all(s["seq_launches"] >= 1 for s in st if s["blocked"])


def test_sequential_path_resumes_across_launches(transfer):
    """A step budget of 40 ball tets: the loop is relaunched from its cursor."""
    st = check_case(transfer, "frag_6_counts", seq_steps=40)
    assert st[0]["blocked"] == 1 and st[0]["seq_launches"] > 10
    st = check_case(transfer, "frag_6_counts", adja=False, seq_steps=1)
    assert st[1]["seq_launches"] >= st[1]["front"]


# ---- 8. unstructured ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wave_bisect", "wave_random"])
def test_unstructured(transfer, name):
    st = check_case(transfer, name)
    assert all(s["blocked"] == 0 for s in st) and st[0]["recolor"] > 0


# ---- 9. three ranks emulated ----------------------------------------------------------------------

def test_three_ranks(transfer):
    m, tg, mp, node, begin, layers, t = F.run("ranks3")
    check_case(transfer, "ranks3")
    mark = transfer.moveifc_marks()
    assert (mark % 3 != 1).any()                                 # tets took foreign colours
    part, ngrp = transfer.moveifc_part(None, N.GRPSPL_DISTR_TARGET)
    ok, tpart, tn = t.part(1)
    assert ok and ngrp == tn and np.array_equal(part, tpart)
    ngr = np.array([2, 3, 4], np.int32)
    part, ngrp = transfer.moveifc_part(mark, N.GRPSPL_DISTR_TARGET, ngr)
    ok, tpart, tn = t.part(1, ngr)
    assert ok and ngrp == tn and np.array_equal(part, tpart)
    out = np.full(m.ne, SENT, np.int32)
    n = C.c_int32(SENT)
    r = transfer.lib.pmx_moveifc_part(transfer.ctx, None, N.GRPSPL_MMG_TARGET, None, out.ctypes.data_as(N.i32ptr),
                                      C.byref(n))
    assert r == 0 and np.all(out == SENT) and n.value == SENT
    assert b"another rank" in transfer.lib.pmx_last_error(transfer.ctx)
    # local marks only: the old groups
    own = np.where(mark % 3 == 1, mark, 4).astype(np.int32)
    part, ngrp = transfer.moveifc_part(own, N.GRPSPL_MMG_TARGET)
    ok, tpart, tn = t.part(2, mark=own)
    assert ok and ngrp == tn == 3 and np.array_equal(part, tpart)


def test_three_ranks_on_the_parallel_path(transfer):
    """Own weights that are no counts: no layer blocks, so foreign colours meet
    the parallel kernels.  Tets are recoloured from foreign colours, and negrp
    loses exactly the recolourings from local colours (the model's D, which
    follows every tet's history), not those from foreign ones."""
    m, tg, mp, node, begin, layers, t = F.run("ranks3_big")
    pts = node[0]
    upload(transfer, m)
    assert transfer.moveifc_begin(tg, mp) == begin["nfront"]
    from_foreign = 0
    for li, (ok, st, snap) in enumerate(layers):
        transfer.moveifc_set_colors(pts, F.exchange_fn(t.weight, node, li)(transfer.moveifc_colors(pts)))
        pre = same_state(transfer, t.pres[li], f"start of layer {li}")
        assert pre["front"][pts - 1].all()
        got = transfer.moveifc_layer()
        assert got["blocked"] == 0 and {k: got[k] for k in TWIN_STATS} == {k: st[k] for k in TWIN_STATS}
        post = same_state(transfer, snap, f"layer {li}")
        _, D, nrec, _, _, nforeign = F.model_layer(m, t, pre)
        changed = post["mark"] != pre["mark"]
        from_foreign += int((changed & (pre["mark"] % 3 != 1)).sum())
        assert np.array_equal(pre["negrp"] - post["negrp"], D)
        assert got["recolor"] == nrec == D.sum() + nforeign
        if got["recolor"] == changed.sum():                      # no tet changed twice: the snapshots count exactly
            local = changed & (pre["mark"] % 3 == 1)
            assert np.array_equal(pre["negrp"] - post["negrp"], np.bincount(pre["mark"][local] // 3, minlength=3))
    assert from_foreign > 0 and len(layers) == 3


def test_a_point_listed_twice_keeps_its_last_colour(transfer):
    m, tg, mp, node, begin, layers, t = F.run("ranks3_big")
    upload(transfer, m)
    transfer.moveifc_begin(tg, mp)
    tt = F.Twin(m, tg, mp)
    ip = np.array([5, 9, 5, 9, 5], np.int32)
    col = np.array([0, 2, 5, 7, 2], np.int32)
    transfer.moveifc_set_colors(ip, col)
    tt.set_colors(ip, col)
    same_state(transfer, tt.snapshot(), "after set_colors")
    assert list(transfer.moveifc_colors(np.array([5, 9], np.int32))) == [2, 7]


# ---- 10. a ball that is not face-connected -----------------------------------------------------------

def test_corner_vertex(transfer):
    m, tg, mp, node, begin, layers, t = F.run("corner")
    _, ne_a, corner = F.two_cubes_corner(2)
    check_case(transfer, "corner")
    assert begin["front"][corner - 1] == 1 and begin["s"][corner - 1] // 4 > ne_a
    at_corner = np.nonzero((m.tet[1:ne_a + 1] == corner).any(1))[0]
    assert np.array_equal(transfer.moveifc_marks()[at_corner], begin["mark"][at_corner])


# ---- 11. overflow -------------------------------------------------------------------------------------

def test_ball_at_the_limit(transfer):
    st = check_case(transfer, "cone_71")
    assert st[0]["maxball"] == 2 * 71 * 71


def test_ball_overflow_leaves_the_layer_start(transfer):
    m, tg, mp, node, begin, layers, t = F.run("cone_72")
    _, apex = F.cone(72)
    assert not layers[0][0] and layers[0][1]["overflow_ip"] == apex
    upload(transfer, m)
    assert transfer.moveifc_begin(tg, mp) == begin["nfront"]
    with pytest.raises(RuntimeError, match=f"point {apex} "):
        transfer.moveifc_layer()
    assert transfer._moveifc_last.overflow_ip == apex
    assert transfer.kernel_ms(LAYER_SLOT) == -1.0
    same_state(transfer, begin, "after the overflow")           # marks still delivered, state untouched


# ---- 12. the chain --------------------------------------------------------------------------------------

def test_chain_merge_adopt_displace_fix_split(transfer):
    m = M.kuhn_cube(6)
    x, y, z = R.cells(m, 6).T
    part = ((x >= 4) + 2 * (y >= 3)).astype(np.int32)
    sp, comm = G.split_case(m, part, 4)
    groups = sp["groups"]
    twin_merge = G.merge(groups, comm)
    mm = M.from_tets(twin_merge["xyz"], twin_merge["tetra_v"])
    mp = F.single_map([g["tetra_v"].shape[0] - 1 for g in groups])
    t = F.Twin(mm, twin_merge["tet_group"], mp)
    transfer.merge_groups(groups, comm)
    transfer.merge_adopt(0)
    assert transfer.moveifc_begin(None, mp) == t.nfront > 0
    same_state(transfer, t.snapshot(), "begin")
    for li in range(2):
        ok, st = t.layer()
        got = transfer.moveifc_layer()
        assert ok and {k: got[k] for k in TWIN_STATS} == {k: st[k] for k in TWIN_STATS}
        same_state(transfer, t.snapshot(), f"layer {li}")
    colors = np.arange(4, dtype=np.int32)                        # nprocs * i + myrank
    fixed, fst = transfer.fix_contiguity(transfer.moveifc_marks(), colors)
    tfixed, tst = R.fix(mm, t.mark.copy(), colors)
    assert np.array_equal(fixed, tfixed) and fst["counter"] == tst["counter"]
    p, ngrp = transfer.moveifc_part(fixed, N.GRPSPL_MMG_TARGET)
    ok, tp, tn = t.part(2, mark=tfixed)
    assert ok and ngrp == tn == 4 and np.array_equal(p, tp)
    p = S.fix_empty(p, ngrp)
    plan = transfer.split_groups(p, ngrp)
    tsp = S.split(mm, p, ngrp)
    assert np.array_equal(plan["sizes"], tsp["sizes"]) and np.array_equal(plan["tet_new"], tsp["tet_new"])
    assert plan["sizes"][:, 0].sum() == mm.ne
    # the adoption of another group drops the displacement
    transfer.merge_adopt(0)
    assert transfer.lib.pmx_moveifc_layer(transfer.ctx, 0, None) == 0


# ---- 13. refusals ---------------------------------------------------------------------------------------

def raw_begin(tr, tg, nprocs, myrank, nold, displs, mapgrp):
    displs, mapgrp = np.ascontiguousarray(displs, np.int32), np.ascontiguousarray(mapgrp, np.int32)
    mp = N.MoveIfcMap(nprocs, myrank, nold, displs.ctypes.data_as(N.iptr), mapgrp.ctypes.data_as(N.iptr))
    nf = C.c_int64(SENT)
    r = tr.lib.pmx_moveifc_begin(tr.ctx, tg.ctypes.data_as(N.i32ptr) if tg is not None else None, C.byref(mp),
                                 C.byref(nf))
    return r, nf.value == SENT, tr.lib.pmx_last_error(tr.ctx)


def test_refusals_leave_outputs_untouched(transfer):
    m = M.kuhn_cube(4)
    tg = R.slabs(m, 2).astype(np.int32)
    cnt = F.counts(tg, 2)
    buf = np.full(max(m.ne, m.np), SENT, np.int32)
    ip = np.array([1, 2], np.int32)

    def before_begin(tr):
        lib, ctx, p = tr.lib, tr.ctx, buf.ctypes.data_as(N.iptr)
        st = N.MoveIfcStats()
        st.front = SENT
        assert lib.pmx_moveifc_layer(ctx, 0, C.byref(st)) == 0 and st.front == SENT
        assert b"pmx_moveifc_begin" in lib.pmx_last_error(ctx)
        assert lib.pmx_moveifc_get_colors(ctx, 2, ip.ctypes.data_as(N.iptr), p) == 0
        assert lib.pmx_moveifc_set_colors(ctx, 2, ip.ctypes.data_as(N.iptr), ip.ctypes.data_as(N.iptr)) == 0
        assert lib.pmx_moveifc_marks(ctx, buf.ctypes.data_as(N.i32ptr)) == 0
        assert lib.pmx_moveifc_points(ctx, p, None, None) == 0
        assert lib.pmx_moveifc_part(ctx, None, 2, None, buf.ctypes.data_as(N.i32ptr), None) == 0
        assert np.all(buf == SENT)
        assert tr.kernel_ms(BEGIN_SLOT) == -1.0 and tr.kernel_ms(LAYER_SLOT) == -1.0

    tr = Transfer(0)
    try:
        r, clean, err = raw_begin(tr, tg, 1, 0, 2, [0, 2], cnt)
        assert r == 0 and clean and b"upload a group first" in err
        before_begin(tr)
    finally:
        tr.close()
    upload(transfer, m)
    before_begin(transfer)
    cases = [
        (b"tet_group outside", dict(tg=np.where(np.arange(m.ne) == 5, 2, tg).astype(np.int32))),
        (b"tet_group outside", dict(tg=np.where(np.arange(m.ne) == 7, -1, tg).astype(np.int32))),
        (b"mapgrp <= 0", dict(mapgrp=[cnt[0], 0])),
        (b"displsgrp", dict(displs=[1, 3])),
        (b"displsgrp", dict(displs=[0, 3], mapgrp=[1, 2, 3])),
        (b"displsgrp", dict(nprocs=2, displs=[0, 3, 2], mapgrp=[1, 2, 3])),
        (b"myrank", dict(myrank=1)),
        (b"no merge plan", dict(tg=None)),
    ]
    transfer.merge_release()
    for what, kw in cases:
        a = dict(tg=tg, nprocs=1, myrank=0, nold=2, displs=[0, 2], mapgrp=cnt)
        a.update(kw)
        r, clean, err = raw_begin(transfer, **a)
        assert r == 0 and clean and what in err, (what, err)
    # a deleted tet
    md = M.Mesh(m.xyz, m.tet.copy(), m.adja, m.tria, m.adjt)
    md.tet[3, 0] = 0
    upload(transfer, md)
    r, clean, err = raw_begin(transfer, tg, 1, 0, 2, [0, 2], cnt)
    assert r == 0 and clean and b"deleted tet" in err
    # a good begin, then the range checks of the colour calls
    upload(transfer, m)
    transfer.moveifc_begin(tg, F.single_map(cnt))
    assert transfer.kernel_ms(BEGIN_SLOT) > 0.0 and transfer.kernel_ms(LAYER_SLOT) == -1.0
    before = state(transfer)
    for bad in (0, m.np + 1):
        pts = np.array([1, bad], np.int32)
        col = np.array([0, 0], np.int32)
        out = np.full(2, SENT, np.int32)
        assert transfer.lib.pmx_moveifc_get_colors(transfer.ctx, 2, pts.ctypes.data_as(N.iptr),
                                                   out.ctypes.data_as(N.iptr)) == 0 and np.all(out == SENT)
        assert transfer.lib.pmx_moveifc_set_colors(transfer.ctx, 2, pts.ctypes.data_as(N.iptr),
                                                   col.ctypes.data_as(N.iptr)) == 0
        assert b"outside 1..np" in transfer.lib.pmx_last_error(transfer.ctx)
    with pytest.raises(RuntimeError, match="colour of no group"):
        transfer.moveifc_set_colors(np.array([1], np.int32), np.array([2], np.int32))
    same_state(transfer, before, "after refused colour calls")
    transfer.moveifc_layer()
    assert transfer.kernel_ms(LAYER_SLOT) > 0.0
    # an upload drops the displacement, as it drops a split plan
    upload(transfer, m)
    buf[:] = SENT
    assert transfer.lib.pmx_moveifc_marks(transfer.ctx, buf.ctypes.data_as(N.i32ptr)) == 0 and np.all(buf == SENT)
    assert transfer.lib.pmx_moveifc_layer(transfer.ctx, 0, None) == 0
    transfer.moveifc_begin(tg, F.single_map(cnt))
    transfer.moveifc_release()
    assert transfer.lib.pmx_moveifc_marks(transfer.ctx, buf.ctypes.data_as(N.i32ptr)) == 0
    assert transfer.kernel_ms(BEGIN_SLOT) == -1.0


def test_move_interfaces_wrapper(transfer):
    m, tg, mp, node, begin, layers, t = F.run("ranks3")
    upload(transfer, m)
    calls = []

    def exchange(colors):
        calls.append(len(calls))
        return F.exchange_fn(t.weight, node, calls[-1])(colors)

    marks, stats = transfer.move_interfaces(tg, mp, nlayers=len(layers), exchange=exchange, node_points=node[0])
    assert len(calls) == len(layers) and stats[0]["nfront"] == begin["nfront"]
    assert np.array_equal(marks, layers[-1][2]["mark"])


# ---- the C driver ------------------------------------------------------------------------------

DEMO_SRC = os.path.join(ROOT, "tests", "c", "moveifc_demo.c")
DEMO_BIN = os.path.join(ROOT, "tests", "c", "_build", "moveifc_demo")


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


def fnv(a) -> int:
    h = 1469598103934665603
    for x in np.asarray(a, np.int32).view(np.uint32).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_driver(transfer):
    r = subprocess.run([build_demo()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "moveifc ok" in r.stdout
    m = M.kuhn_cube(6)
    tg = (1 - 2 * np.arange(m.ne) // m.ne).astype(np.int32)
    t = F.Twin(m, tg, F.single_map([300, 900]))
    recolor = 0
    for _ in range(2):
        ok, st = t.layer()
        assert ok
        recolor += st["recolor"]
    colors = np.arange(2, dtype=np.int32)
    fixed, _ = R.fix(m, t.mark.copy(), colors)
    ok, part, ngrp = t.part(2, mark=fixed)
    assert ok and ngrp == 2
    sp = S.split(m, part, ngrp)
    line = next(l for l in r.stdout.splitlines() if l.startswith("moveifc ne="))
    want = (f"moveifc ne={m.ne} nfront={t.nfront} recolor={recolor} marks={fnv(t.mark):016x} "
            f"fixed={fnv(fixed):016x} part={fnv(part):016x} tet_new={fnv(sp['tet_new']):016x}")
    assert line == want
