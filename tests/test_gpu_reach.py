"""pmx_reach_face_marks / pmx_check_reachability / pmx_moveifc_fix /
pmx_moveifc_reach on the GPU against the CPU twin (tests/c/reach_ref.c):
PMMG_fix_contiguity and steps 2-3 of PMMG_check_reachability (reference
src/moveinterfaces_pmmg.c:377-523, 627-811).

Marks and counter are compared byte for byte, the stats in every field the
twin has.  The twin's results are computed once per case (reach_ref.case) and
shared."""
import ctypes as C

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

SENT = -77
REACH_SLOT, FIX_SLOT = 22, 23


def upload(tr, m, adja=True):
    tr.upload_background(m, [np.ones((m.np + 1, 1))], 0, adja=adja)


def check_case(tr, name, adja=True, replay_steps=0):
    """The device's fix and check equal the twin's; returns the check's stats."""
    d = X.case(name)
    upload(tr, d["m"], adja)
    fixed, fst = tr.fix_contiguity(d["mark0"], X.COLORS)
    assert fixed.tobytes() == d["fixed"].tobytes() and fst["counter"] == d["fix_counter"]
    sent = tr.reach_face_marks(fixed, d["fi"])
    assert sent.dtype == np.int32 and np.array_equal(sent, fixed[d["fi"] // 12 - 1])
    got, counter, st = tr.check_reachability(fixed, X.COLORS, d["fi"], d["cin"], fst["counter"], replay_steps)
    print(name, st)
    assert got.dtype == np.int32 and got.tobytes() == d["mark"].tobytes()
    assert counter == d["stats"]["counter"] == st["counter"]
    assert {k: st[k] for k in X.REACH_FIELDS} == {k: d["stats"][k] for k in X.REACH_FIELDS}
    assert st["rounds"] == (st["nrescanned"] + 1 if st["nunreached"] else 0) and st["relabels"] == st["nrescanned"]
    assert tr.kernel_ms(REACH_SLOT) > 0.0
    return st


# ---- 1. - 8., 10. the planted cases -----------------------------------------------------------

@pytest.mark.parametrize("name", [c for c in X.CASES if c not in X.RANDOM_CASES])
def test_planted_cases(transfer, name):
    st = check_case(transfer, name)
    d = X.case(name)
    if name in ("local4", "reached6"):
        assert st["nunreached"] == 0 and st["replays"] == 0 and d["mark"].tobytes() == d["fixed"].tobytes()
    if name == "two_cubes@small_unset":
        assert st["ncannot"] == 1
    if name in ("nested6", "beside6"):
        assert st["nrescanned"] >= 1 and st["rounds"] >= 2


# ---- 9. random marks, random colours received ---------------------------------------------------

@pytest.mark.parametrize("name", X.RANDOM_CASES)
def test_random_cases(transfer, name):
    st = check_case(transfer, name)
    assert st["nrescanned"] > 0


# ---- mechanics --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nested6", "random_4_1", "two_cubes@small_unset"])
def test_one_dequeue_per_launch(transfer, name):
    a = check_case(transfer, name)
    b = check_case(transfer, name, replay_steps=1)
    assert b["replay_steps"] == a["replay_steps"] and b["replays"] > a["replays"]


def test_two_runs_give_identical_bytes(transfer):
    d = X.case("random_6_2")
    upload(transfer, d["m"])
    runs = [transfer.check_reachability(d["fixed"], X.COLORS, d["fi"], d["cin"], d["fix_counter"]) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1:] == runs[1][1:]


@pytest.mark.parametrize("name", ["fragments6", "random_6_1", "wave"])
def test_device_built_adjacency(transfer, name):
    check_case(transfer, name, adja=False)


def test_entry_order_does_not_matter(transfer):
    d = X.case("fragments6@dup")
    upload(transfer, d["m"])
    perm = np.random.default_rng(2).permutation(len(d["fi"]))
    got, counter, st = transfer.check_reachability(d["fixed"], X.COLORS, d["fi"][perm], d["cin"][perm],
                                                   d["fix_counter"])
    assert got.tobytes() == d["mark"].tobytes() and st["nseeds"] == d["stats"]["nseeds"]


def test_no_entries(transfer):
    d = X.case("reached6@unset")
    upload(transfer, d["m"])
    none = np.zeros(0, np.int32)
    got, counter, st = transfer.check_reachability(d["fixed"], X.COLORS, none, none, d["fix_counter"])
    assert got.tobytes() == d["mark"].tobytes() and counter == d["m"].ne
    assert len(transfer.reach_face_marks(d["fixed"], none)) == 0


# ---- the chain, in place on the device --------------------------------------------------------

def twin_tail(mm, t, fi, rank):
    """The twin's fix and check on the displacement twin's marks."""
    colors = (t.nprocs * np.arange(t.nold) + t.myrank).astype(np.int32)
    w = X.Twin(mm, t.mark.copy())
    fixed, fst = w.fix(colors)
    c = fixed[fi // 12 - 1]
    cin = np.where(c % t.nprocs == rank, c, X.UNSET).astype(np.int32) if t.nprocs > 1 else np.full(len(fi), X.UNSET,
                                                                                                   np.int32)
    ok, out, st = w.reach(fi, cin)
    assert ok
    return fixed, fst, cin, out, st


def device_tail(tr, t, fi, rank, fixed, fst, cin, out, st):
    """fix, face marks, check and part on the device's own marks: nothing of
    size ne goes in."""
    gst = tr.moveifc_fix()
    assert gst["counter"] == fst["counter"] and gst["nmerged"] == fst["fix_nmerged"]
    assert tr.kernel_ms(FIX_SLOT) > 0.0
    assert tr.moveifc_marks().tobytes() == fixed.tobytes()
    sent = tr.reach_face_marks(None, fi)
    assert np.array_equal(sent, fixed[fi // 12 - 1])
    got_cin = (np.where(sent % t.nprocs == rank, sent, X.UNSET).astype(np.int32) if t.nprocs > 1 else
               np.full(len(fi), X.UNSET, np.int32))
    assert np.array_equal(got_cin, cin)
    rst = tr.moveifc_reach(fi, got_cin)
    print(rst)
    assert {k: rst[k] for k in X.REACH_FIELDS} == {k: st[k] for k in X.REACH_FIELDS}
    assert tr.moveifc_marks().tobytes() == out.tobytes()
    # a second check wants a fix first
    assert tr.lib.pmx_moveifc_reach(tr.ctx, 0, None, None, 0, None) == 0
    assert b"pmx_moveifc_fix" in tr.lib.pmx_last_error(tr.ctx)
    return rst


def test_chain_merge_adopt_displace_fix_reach_split(transfer):
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
    for _ in range(2):
        assert t.layer()[0]
        transfer.moveifc_layer()
    fi, rank = X.entries(mm, 1 / 6)
    tail = twin_tail(mm, t, fi, rank)
    rst = device_tail(transfer, t, fi, rank, *tail)
    assert rst["counter"] == mm.ne and rst["nunreached"] == 0       # one rank: every colour is its own
    p, ngrp = transfer.moveifc_part(None, N.GRPSPL_MMG_TARGET)
    ok, tp, tn = t.part(2, mark=tail[3])
    assert ok and ngrp == tn == 4 and np.array_equal(p, tp)
    p = S.fix_empty(p, ngrp)
    plan = transfer.split_groups(p, ngrp)
    tsp = S.split(mm, p, ngrp)
    assert np.array_equal(plan["sizes"], tsp["sizes"]) and np.array_equal(plan["tet_new"], tsp["tet_new"])


def test_chain_three_ranks(transfer):
    m, tg, mp, node, begin, layers, t0 = F.run("ranks3")
    t = F.Twin(m, tg, mp)
    upload(transfer, m)
    transfer.moveifc_begin(tg, mp)
    for li in range(len(layers)):
        pts = node[0]
        t.set_colors(pts, F.exchange_fn(t.weight, node, li)(t.colors(pts)))
        transfer.moveifc_set_colors(pts, F.exchange_fn(t.weight, node, li)(transfer.moveifc_colors(pts)))
        assert t.layer()[0]
        transfer.moveifc_layer()
    assert transfer.moveifc_marks().tobytes() == t.mark.tobytes()
    assert (~np.isin(t.mark, [1, 4, 7])).any()                      # foreign colours after the layers
    fi, rank = X.entries(m, 1 / 6)
    tail = twin_tail(m, t, fi, rank)
    rst = device_tail(transfer, t, fi, rank, *tail)
    assert rst["counter"] == m.ne
    ngrps = np.diff(mp["displsgrp"]).astype(np.int32)
    p, ngrp = transfer.moveifc_part(None, N.GRPSPL_DISTR_TARGET, ngrps)
    ok, tp, tn = t.part(1, ngrps, mark=tail[3])
    assert ok and ngrp == tn and np.array_equal(p, tp)
    p = S.fix_empty(p, ngrp)
    plan = transfer.split_groups(p, ngrp)
    tsp = S.split(m, p, ngrp)
    assert np.array_equal(plan["sizes"], tsp["sizes"]) and np.array_equal(plan["tet_new"], tsp["tet_new"])
    # a layer after the fix wants a new fix before the check
    transfer.moveifc_fix()
    transfer.moveifc_layer()
    assert transfer.lib.pmx_moveifc_reach(transfer.ctx, 0, None, None, 0, None) == 0


# ---- refusals -----------------------------------------------------------------------------------

def raw_reach(tr, mark, colors, fi, cin, counter=True, nface=None, steps=0):
    """(return value, outputs untouched, error)."""
    st = N.ReachStats()
    st.counter = SENT
    cnt = C.c_int64(SENT)
    before = None if mark is None else mark.copy()
    col = np.ascontiguousarray(colors, np.int32)
    r = tr.lib.pmx_check_reachability(
        tr.ctx, mark.ctypes.data_as(N.i32ptr) if mark is not None else None, len(col), col.ctypes.data_as(N.i32ptr),
        len(fi) if nface is None else nface, fi.ctypes.data_as(N.iptr) if fi is not None else None,
        cin.ctypes.data_as(N.i32ptr) if cin is not None else None, C.byref(cnt) if counter else None, steps,
        C.byref(st))
    clean = cnt.value == SENT and st.counter == SENT and (mark is None or np.array_equal(mark, before))
    return r, clean, tr.lib.pmx_last_error(tr.ctx)


def test_refusals_leave_outputs_untouched(transfer):
    d = X.case("fragments6")
    m, fi, cin = d["m"], d["fi"], d["cin"]
    mark = d["fixed"].copy()
    out = np.full(len(fi), SENT, np.int32)
    outp = out.ctypes.data_as(N.i32ptr)

    tr = Transfer(0)
    try:
        r, clean, err = raw_reach(tr, mark, X.COLORS, fi, cin)
        assert r == 0 and clean and b"upload a group first" in err
        assert tr.lib.pmx_reach_face_marks(tr.ctx, mark.ctypes.data_as(N.i32ptr), len(fi), fi.ctypes.data_as(N.iptr),
                                           outp) == 0
        assert tr.lib.pmx_moveifc_fix(tr.ctx, 0, None) == 0 and b"pmx_moveifc_begin" in tr.lib.pmx_last_error(tr.ctx)
        assert tr.lib.pmx_moveifc_reach(tr.ctx, 0, None, None, 0, None) == 0
        assert tr.kernel_ms(REACH_SLOT) == -1.0 and tr.kernel_ms(FIX_SLOT) == -1.0
    finally:
        tr.close()

    upload(transfer, m)
    bad = fi.copy()
    for case, kw, word in [
        ("nface < 0", dict(fi=fi, cin=cin, nface=-1), b"nface"),
        ("NULL face_index1", dict(fi=None, cin=cin, nface=3), b"NULL"),
        ("NULL color_in", dict(fi=fi, cin=None), b"NULL"),
        ("counter NULL", dict(fi=fi, cin=cin, counter=False), b"counter"),
        ("replay_steps < 0", dict(fi=fi, cin=cin, steps=-1), b"replay_steps"),
    ]:
        r, clean, err = raw_reach(transfer, mark, X.COLORS, kw.pop("fi"), kw.pop("cin"), **kw)
        assert r == 0 and clean and word in err, case
        assert transfer.kernel_ms(REACH_SLOT) == -1.0
    for tet in (0, m.ne + 1):
        bad[3] = 12 * tet + 5
        r, clean, err = raw_reach(transfer, mark, X.COLORS, bad, cin)
        assert r == 0 and clean and b"outside 1..ne" in err
        assert transfer.lib.pmx_reach_face_marks(transfer.ctx, mark.ctypes.data_as(N.i32ptr), len(bad),
                                                 bad.ctypes.data_as(N.iptr), outp) == 0
    r, clean, err = raw_reach(transfer, mark, [1, 4, 1], fi, cin)
    assert r == 0 and clean and b"duplicate colours" in err
    r, clean, err = raw_reach(transfer, None, X.COLORS, fi, cin)
    assert r == 0 and clean and b"mark is NULL" in err
    # the device's marks, without a displacement
    assert transfer.lib.pmx_reach_face_marks(transfer.ctx, None, len(fi), fi.ctypes.data_as(N.iptr), outp) == 0
    assert b"pmx_moveifc_begin" in transfer.lib.pmx_last_error(transfer.ctx)
    assert transfer.lib.pmx_reach_face_marks(transfer.ctx, mark.ctypes.data_as(N.i32ptr), -1, None, outp) == 0
    assert np.all(out == SENT)
    # after all that the call still works
    got, counter, st = transfer.check_reachability(mark, X.COLORS, fi, cin, d["fix_counter"])
    assert got.tobytes() == d["mark"].tobytes()


def test_moveifc_refusals_leave_the_device_marks(transfer):
    m, tg, mp, node, begin, layers, t0 = F.run("ranks3")
    upload(transfer, m)
    transfer.moveifc_begin(tg, mp)
    transfer.moveifc_set_colors(node[0], F.exchange_fn(t0.weight, node, 0)(transfer.moveifc_colors(node[0])))
    transfer.moveifc_layer()
    before = transfer.moveifc_marks()
    fi, rank = X.entries(m, 1 / 6)
    cin = np.full(len(fi), X.UNSET, np.int32)
    lib, ctx = transfer.lib, transfer.ctx
    st = N.ReachStats()
    st.counter = SENT
    fip, cp = fi.ctypes.data_as(N.iptr), cin.ctypes.data_as(N.i32ptr)
    assert lib.pmx_moveifc_reach(ctx, len(fi), fip, cp, 0, C.byref(st)) == 0           # no fix yet
    assert b"pmx_moveifc_fix" in lib.pmx_last_error(ctx) and st.counter == SENT
    cs = N.ContigStats()
    cs.counter = SENT
    assert lib.pmx_moveifc_fix(ctx, -1, C.byref(cs)) == 0 and cs.counter == SENT
    assert transfer.kernel_ms(FIX_SLOT) == -1.0
    assert transfer.moveifc_marks().tobytes() == before.tobytes()
    transfer.moveifc_fix()
    fixed = transfer.moveifc_marks()
    bad = fi.copy()
    bad[0] = 12 * (m.ne + 1)
    for args in [(-1, fip, cp, 0), (len(fi), None, cp, 0), (len(fi), fip, None, 0), (len(fi), fip, cp, -1),
                 (len(bad), bad.ctypes.data_as(N.iptr), cp, 0)]:
        assert lib.pmx_moveifc_reach(ctx, *args, C.byref(st)) == 0 and st.counter == SENT
        assert transfer.kernel_ms(REACH_SLOT) == -1.0
        assert transfer.moveifc_marks().tobytes() == fixed.tobytes()
    rst = transfer.moveifc_reach(fi, cin)                                              # the fix still counts
    assert rst["counter"] == m.ne
    # set_colors after a fix: the check wants a new fix
    transfer.moveifc_fix()
    transfer.moveifc_set_colors(node[0][:1], transfer.moveifc_colors(node[0][:1]))
    assert lib.pmx_moveifc_reach(ctx, len(fi), fip, cp, 0, None) == 0
    # a new background drops the displacement
    upload(transfer, m)
    assert lib.pmx_moveifc_fix(ctx, 0, None) == 0 and transfer.kernel_ms(FIX_SLOT) == -1.0
