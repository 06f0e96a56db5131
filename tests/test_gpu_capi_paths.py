"""Host paths of the C ABI's results and new-tet calls that only a partial
request reaches: pmx_download asked for a part of the results (after a plain
and after a PMX_RUN_EAGER_DOWNLOAD step), pmx_upload_new_tets re-sending the
view's tets with deleted rows among them, and a step on zero points.

The downloads use the 6-cube case of test_eager_download_equals_download: NUL
points, and new tets that leave 15 % of the points orphaned (so that the
orphan reset, and the eager path's second copy of the masks, run).
"""
import ctypes as C

import numpy as np
import pytest

from helpers import bits_equal, cube_case
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu


def _orphan_case():
    m, x, t, sols = cube_case(6, metric="iso", surface=True)
    n = len(x)
    t = t.copy()
    t[5::41] = M.TAG_NUL
    rng = np.random.default_rng(11)
    used = np.zeros(n, bool)
    used[: int(0.85 * n)] = True
    pool = np.nonzero(used)[0]
    tets = np.zeros((len(pool) + 1, 4), np.int32)
    tets[1:] = rng.choice(pool, size=(len(pool), 4))
    tets[1:, 0] = pool
    tets[0] = -1
    return m, x, t, sols, tets


@pytest.mark.parametrize("flags", [0, N.RUN_EAGER_DOWNLOAD], ids=["plain", "eager"])
def test_partial_downloads_equal_the_full_one(transfer, flags):
    """The fields only, the three int arrays only, and each int array alone:
    every answer is, bit for bit, that part of a full download of the same
    step, and what was not asked for is not written."""
    m, x, t, sols, tets = _orphan_case()
    n = len(x)
    transfer.upload_background(m, sols, 0)
    transfer.upload_points(x, t, tets)
    transfer.run(flags=flags)
    fresh = lambda: [np.full((n, s.shape[1]), -7.0) for s in sols]
    full = transfer.download(init=fresh())
    assert (full.status != 0).any() and (full.elem == 0).any()

    only = transfer.download(init=fresh(), sols_only=True)
    for s in range(len(sols)):
        assert bits_equal(only.sols[s], full.sols[s]).all()
    assert not only.elem.any() and not only.status.any() and not only.steps.any()

    lib, ctx = transfer.lib, transfer.ctx
    ip = lambda a: a.ctypes.data_as(N.iptr)
    want = {"elem": full.elem, "status": full.status, "steps": full.steps}
    for asked in (("elem", "status", "steps"), ("elem",), ("status",), ("steps",)):
        got = {k: np.full(n, -5, np.int32) for k in want}
        args = [ip(got[k]) if k in asked else None for k in ("elem", "status", "steps")]
        assert lib.pmx_download(ctx, None, n, *args) == 1, lib.pmx_last_error(ctx).decode()
        for k in want:
            if k in asked:
                assert np.array_equal(got[k], want[k]), (asked, k)
            else:
                assert np.all(got[k] == -5), (asked, k)
    # and the full download once more, after the partial ones
    again = transfer.download(init=fresh())
    for s in range(len(sols)):
        assert bits_equal(again.sols[s], full.sols[s]).all()
    assert np.array_equal(again.elem, full.elem) and np.array_equal(again.steps, full.steps)


def test_resent_view_tets_with_deleted_rows():
    """pmx_upload_new_tets after a step whose view carried tets, with the same
    tets (deleted rows, v[0] <= 0, among them): accepted, and the new mesh's
    qualities and the promoted background are those of the run that never
    re-sent them.  (A jittered Kuhn cube with the tets around its last 15 % of
    vertices deleted, not random tets: a promotion matches the tets' faces.)"""
    m1 = M.kuhn_cube(6, seed=11)
    sols1 = [M.on_vertices(m1, M.shock_metric), M.on_vertices(m1, M.level_set)]
    m2 = M.kuhn_cube(5, seed=22)
    x2 = m2.xyz[1:].copy()
    n = len(x2)
    onb = np.any((x2 == 0.0) | (x2 == 1.0), axis=1)
    t2 = np.where(onb, M.TAG_BDY, 0).astype(np.uint16)
    tets0 = m2.tet.copy() - 1
    tets0[0] = -1
    dead = np.any(tets0 >= int(0.85 * n), axis=1)
    dead[0] = False
    tets0[dead, 0] = -1
    assert 0 < dead.sum() < m2.ne
    live = np.zeros(n, bool)
    live[tets0[1:][~dead[1:]].ravel()] = True
    assert (~live).any()
    init = [np.full((n, s.shape[1]), 0.5) for s in sols1]

    def cycle(resend):
        tr = Transfer(0)
        try:
            tr.upload_background(m1, sols1, 0)
            tr.upload_points(x2, t2, tets0)
            tr.run()
            r = tr.download(init=init)
            if resend:
                tr.upload_new_tets(tets0)
                r_again = tr.download(init=init)
                assert np.array_equal(r.elem, r_again.elem)
            q = tr.new_mesh_qual(None)
            tr.promote_background(m2, r.sols, adja=False)
            return r, q, tr.tetra_qual(m2.ne)
        finally:
            tr.close()

    ra, qa, ba = cycle(False)
    rb, qb, bb = cycle(True)
    assert np.all(ra.elem[~live] == 0) and np.all(ra.status[live & (t2 == 0)] != 0)
    assert np.array_equal(ra.elem, rb.elem) and np.array_equal(ra.status, rb.status)
    for s in range(len(sols1)):
        assert bits_equal(ra.sols[s], rb.sols[s]).all()
        assert np.all(ra.sols[s][~live] == 0.5)
    assert bits_equal(qa.reshape(-1, 1), qb.reshape(-1, 1)).all()
    assert bits_equal(ba.reshape(-1, 1), bb.reshape(-1, 1)).all()
    assert (qa[1:][~dead[1:]] > 0).all()


def test_step_on_zero_points(transfer):
    """A points view with first = 1, last = 0: the step runs, every results
    call returns 1 and writes nothing."""
    m, x, t, sols = cube_case(5, metric="iso", surface=True)
    transfer.upload_background(m, sols, 0)
    transfer.upload_points(np.zeros((0, 3)), np.zeros(0, np.uint16))
    transfer.run()
    lib, ctx = transfer.lib, transfer.ctx
    assert lib.pmx_step_ready(ctx) == 1
    ip = lambda a: a.ctypes.data_as(N.iptr)
    guard = [np.full(8, -5, np.int32) for _ in range(3)]
    views = (N.SolView * len(sols))()
    arrs = [np.full(8 * s.shape[1], -5.0) for s in sols]
    for i, (a, s) in enumerate(zip(arrs, sols)):
        views[i].size, views[i].m = s.shape[1], a.ctypes.data_as(N.dptr)
    err = lambda: lib.pmx_last_error(ctx).decode()
    assert lib.pmx_download(ctx, views, 0, ip(guard[0]), ip(guard[1]), ip(guard[2])) == 1, err()
    assert lib.pmx_download_starts(ctx, ip(guard[0]), 0) == 1, err()
    assert lib.pmx_download_border(ctx, ip(guard[1]), ip(guard[2]), 0) == 1, err()
    assert all(np.all(g == -5) for g in guard) and all(np.all(a == -5.0) for a in arrs)
    st = transfer.locate_stats()
    assert st["nvol"] == 0 and st["nbdy"] == 0 and st["nexhaust"] == 0 and st["nclosest"] == 0
    for path in (0, 1):
        ws = transfer.wave_stats(path)
        assert ws["waves"] == 0 and ws["located"] == 0
    r = transfer.download()
    assert len(r.elem) == 0
    # the context serves a normal step afterwards
    transfer.upload_points(x, t)
    transfer.run()
    assert np.all(transfer.download().status[t == 0] != 0)
