"""CPU: PMX_copyMetricsAndFields_point with more fields than the fused step
carries (a host loop over any number of solutions; no context, no GPU).

PMMG_copyMetricsAndFields_point (reference src/interpmesh_pmmg.c:311-446)
copies the metric and every field of the frozen (MG_REQ) valid old points,
through permNodGlob when the mesh was renumbered; it loops `for j < nsols`
without a limit of its own.
"""
import ctypes as C

import numpy as np
import pytest

from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import mesh_view

NFIELDS = 12
SENT = -7.0


def _views(arrs):
    v = (N.SolView * len(arrs))()
    for i, a in enumerate(arrs):
        v[i].size, v[i].m = a.shape[1], a.ctypes.data_as(N.dptr)
    return v


@pytest.mark.parametrize("with_perm", [False, True])
def test_copy_point_twelve_fields(with_perm):
    lib = N.load()
    m = M.kuhn_cube(4)
    rng = np.random.default_rng(21)
    otag = np.zeros(m.np + 1, np.uint16)
    otag[1::3] = M.TAG_REQ
    otag[2::7] |= M.TAG_BDY
    otag[4::9] = M.TAG_NUL | M.TAG_REQ                       # !MG_VOK: never copied
    sizes = [1] + [(1, 3, 6)[k % 3] for k in range(NFIELDS)]  # the metric, then the fields
    olds = [rng.normal(size=(m.np + 1, sz)) for sz in sizes]
    perm = np.zeros(m.np + 1, np.int32)
    perm[1:] = rng.permutation(m.np) + 1
    news = [np.full((m.np + 1, sz), SENT) for sz in sizes]
    ov, nv = _views(olds), _views(news)
    G = N.Group()
    G.old_mesh = mesh_view(m)
    G.met, G.old_met = C.pointer(nv[0]), C.pointer(ov[0])
    G.nsols = NFIELDS
    G.fields = C.cast(C.byref(nv, C.sizeof(N.SolView)), C.POINTER(N.SolView))
    G.old_fields = C.cast(C.byref(ov, C.sizeof(N.SolView)), C.POINTER(N.SolView))
    r = lib.PMX_copyMetricsAndFields_point(None, C.byref(G), otag.ctypes.data_as(N.u16ptr), 2,
                                           perm.ctypes.data_as(N.iptr) if with_perm else None,
                                           1 if with_perm else 0, 1)
    assert r == 1, lib.pmx_last_error(None).decode()
    want = [np.full((m.np + 1, sz), SENT) for sz in sizes]
    ncopied = 0
    for ip in range(1, m.np + 1):
        if otag[ip] >= M.TAG_NUL or not (otag[ip] & M.TAG_REQ):
            continue
        dst = perm[ip] if with_perm else ip
        for w, o in zip(want, olds):
            w[dst] = o[ip]
        ncopied += 1
    assert 0 < ncopied < m.np
    for k, (a, w) in enumerate(zip(news, want)):
        assert np.array_equal(a, w), f"solution {k} (size {sizes[k]})"
