"""The CPU twin of pmx_metis_graph (tests/c/metis_graph_ref.c) through ctypes,
and the inputs the graph tests share (test infrastructure)."""
import ctypes as C
import os
import subprocess

import numpy as np


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "metis_graph_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libmetis_graph_ref.so")

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["gcc", "-O3", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math",
                            "-fPIC", "-shared", SRC, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, LIB)
        l = C.CDLL(LIB)
        vp, i64 = C.c_void_p, C.c_int64
        l.mgr_graph.restype = i64
        l.mgr_graph.argtypes = [i64, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        l.mgr_face_weights.restype = None
        l.mgr_face_weights.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, i64, vp, vp]
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _met(met):
    if met is None:
        return None, 0
    a = np.ascontiguousarray(met, np.float64)
    return a, (a.shape[1] if a.ndim == 2 else 1)


def graph(m, met=None, met_rid_typ=0, tags=None, weights=True, lengths=True):
    """dict(xadj, adjncy, wgt (double), iwgt, len (n, 4): the lengths of each
    entry's face in MMG5_iarf order and its weight before the clamp; lengths
    False: left out) of mesh m in metric met ((np+1,) or (np+1, 1) iso,
    (np+1, 6) tensor, None: no metric)."""
    a, msize = _met(met)
    t = None if tags is None else np.ascontiguousarray(tags, np.uint16)
    ne = m.ne
    xyz = np.ascontiguousarray(m.xyz, np.float64)
    tet = np.ascontiguousarray(m.tet, np.int32)
    adja = np.ascontiguousarray(m.adja, np.int32)
    xadj = np.zeros(ne + 1, np.int32)
    adjncy = np.zeros(4 * ne + 1, np.int32)
    wgt = np.zeros(4 * ne + 1) if weights else None
    iwgt = np.zeros(4 * ne + 1, np.int32) if weights else None
    ln = np.zeros((4 * ne + 1, 4)) if weights and lengths else None
    n = lib().mgr_graph(ne, _p(xyz), _p(tet), _p(adja), _p(a), msize, met_rid_typ, _p(t), _p(xadj), _p(adjncy),
                        _p(wgt), _p(iwgt), _p(ln))
    cut = lambda x: None if x is None else x[:n]
    return dict(xadj=xadj, adjncy=cut(adjncy), wgt=cut(wgt), iwgt=cut(iwgt), len=cut(ln), n=int(n))


def face_weights(m, faces, met=None, met_rid_typ=0, tags=None):
    a, msize = _met(met)
    t = None if tags is None else np.ascontiguousarray(tags, np.uint16)
    f = np.ascontiguousarray(faces, np.int32)
    xyz = np.ascontiguousarray(m.xyz, np.float64)
    tet = np.ascontiguousarray(m.tet, np.int32)
    w = np.zeros(len(f))
    lib().mgr_face_weights(_p(xyz), _p(tet), _p(a), msize, met_rid_typ, _p(t), len(f), _p(f), _p(w))
    return w


def iso_sizes(m, n):
    """h = (0.5 + 2 x0) / n on the vertices: lengths on both sides of 1."""
    h = np.ones((m.np + 1, 1))
    h[1:, 0] = (0.5 + 2.0 * m.xyz[1:, 0]) / n
    return h


def rotated_tensor(m, n):
    """R diag(1 / h_i^2) R^T with h_i around the cube's edge length 1 / n,
    varying along x (and the rotation with z): a full tensor whose lengths
    fall on both sides of 1."""
    x, y, z = m.xyz[:, 0], m.xyz[:, 1], m.xyz[:, 2]
    s = (0.5 + 2.0 * x) / n
    h = np.stack([0.8 * s, 1.0 * s, 1.3 * s * (1.0 + 0.2 * y)], 1)
    a, b = 0.7 + 0.5 * z, 0.3 + 0.4 * y
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    R = np.zeros((len(x), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = ca * cb, -sa, ca * sb
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = sa * cb, ca, sa * sb
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sb, 0.0, cb
    D = 1.0 / h ** 2
    T = np.einsum("nij,nj,nkj->nik", R, D, R)
    met = np.stack([T[:, 0, 0], T[:, 0, 1], T[:, 0, 2], T[:, 1, 1], T[:, 1, 2], T[:, 2, 2]], 1)
    met[0] = [1, 0, 0, 1, 0, 1]
    return np.ascontiguousarray(met)


def borderline(raw, rel=1e-9):
    """Entries whose weight before the clamp is within rel (relative) of an
    integer or of the clamp: the device's exp may differ from glibc's in the
    last ulp, which only there can change the integer weight."""
    w = np.asarray(raw)
    near_int = (w < 1000000.0 * (1.0 + rel)) & (np.abs(w - np.rint(w)) <= rel * w)
    near_clamp = np.abs(w - 1000000.0) <= rel * 1000000.0
    return near_int | near_clamp


def numpy_graph(m):
    """xadj / adjncy straight from m.adja."""
    ne = m.ne
    a = m.adja[1:4 * ne + 1].reshape(ne, 4) // 4
    on = a != 0
    xadj = np.zeros(ne + 1, np.int32)
    xadj[1:] = np.cumsum(on.sum(1))
    return xadj, (a[on] - 1).astype(np.int32)
