"""The CPU twin of pmx_split_groups / pmx_split_fetch (tests/c/split_ref.c)
through ctypes, and the meshes and partitions the split tests share (test
infrastructure).  The twin is UNPINNED: Mmg is absent, so the reference file it
restates (src/grpsplit_pmmg.c) cannot be built here; tests/test_split_cpu.py
checks it by properties instead."""
import ctypes as C
import os
import subprocess
import time

import numpy as np

import contiguity_ref as R
from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "split_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libsplit_ref.so")

IDIR = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])
INT_KEYS = ("tet_old", "tetra_v", "adja", "point_old", "face_index1", "face_index2", "node_index1", "node_index2")

_lib = None


class Sizes(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("ne", "np", "nface", "nnode")]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", tmp],
                           check=True)
            os.replace(tmp, LIB)
        l = C.CDLL(LIB)
        vp, i64 = C.c_void_p, C.c_int64
        l.spr_split.restype = C.c_int
        l.spr_split.argtypes = [i64, i64, vp, vp, vp, C.c_int, i64, vp, vp, i64, vp, vp,
                                C.POINTER(i64), C.POINTER(i64), vp] + [vp] * 9
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _comm(comm):
    """comm dict (or None) -> (face1, face2, node1, node2, face nitem, node nitem)."""
    comm = comm or {}
    i32 = lambda k: np.ascontiguousarray(comm.get(k, np.zeros(0)), np.int32)
    return (i32("face_index1"), i32("face_index2"), i32("node_index1"), i32("node_index2"),
            int(comm.get("int_face_nitem", 0)), int(comm.get("int_node_nitem", 0)))


def split(m, part, ngrp, comm=None, data=None):
    """The split of mesh m by part: a dict with sizes ((ngrp, 4) int64: ne, np,
    nface, nnode), tet_new, int_face_nitem, int_node_nitem and groups, a list
    of dicts with the arrays Transfer.split_fetch returns (xyz and sols rows
    when data = (xyz, [sols]) is given); seconds: the C call alone."""
    ne, np_ = m.ne, m.np
    tet = np.ascontiguousarray(m.tet, np.int32)
    adja = np.ascontiguousarray(m.adja, np.int32)
    p = np.ascontiguousarray(part, np.int32)
    f1, f2, n1, n2, fn, nn = _comm(comm)
    fn_, nn_ = C.c_int64(fn), C.c_int64(nn)
    sizes = (Sizes * ngrp)()
    cap = 4 * ne + 4
    tet_new, tet_old = np.zeros(ne, np.int32), np.zeros(ne, np.int32)
    tv, ad = np.zeros(4 * ne, np.int32), np.zeros(4 * ne, np.int32)
    pold, of1, of2, on1, on2 = (np.zeros(cap, np.int32) for _ in range(5))
    fn = lib().spr_split
    t0 = time.perf_counter()
    ok = fn(ne, np_, _p(tet), _p(adja), _p(p), ngrp, len(f1), _p(f1), _p(f2), len(n1), _p(n1), _p(n2),
                         C.byref(fn_), C.byref(nn_), C.cast(sizes, C.c_void_p), _p(tet_new), _p(tet_old), _p(tv),
                         _p(ad), _p(pold), _p(of1), _p(of2), _p(on1), _p(on2))
    seconds = time.perf_counter() - t0
    if not ok:
        raise RuntimeError("spr_split: an empty part")
    sz = np.array([[s.ne, s.np, s.nface, s.nnode] for s in sizes], np.int64).reshape(ngrp, 4)
    groups = []
    to = po = fo = no = 0
    for g in range(ngrp):
        neg, npg, nf, nnd = (int(v) for v in sz[g])
        tvg = np.zeros((neg + 1, 4), np.int32)
        tvg[1:] = tv[4 * to:4 * (to + neg)].reshape(neg, 4)
        adg = np.zeros(4 * neg + 5, np.int32)
        adg[1:4 * neg + 1] = ad[4 * to:4 * (to + neg)]
        d = {"tet_old": tet_old[to:to + neg].copy(), "tetra_v": tvg, "adja": adg,
             "point_old": pold[po:po + npg].copy(),
             "face_index1": of1[fo:fo + nf].copy(), "face_index2": of2[fo:fo + nf].copy(),
             "node_index1": on1[no:no + nnd].copy(), "node_index2": on2[no:no + nnd].copy()}
        if data is not None:
            xyz, sols = data
            d["xyz"] = np.zeros((npg + 1, 3))
            d["xyz"][1:] = xyz[d["point_old"]]
            d["sols"] = []
            for s in sols:
                o = np.zeros((npg + 1, s.shape[1]))
                o[1:] = s[d["point_old"]]
                d["sols"].append(o)
        groups.append(d)
        to, po, fo, no = to + neg, po + npg, fo + nf, no + nnd
    return {"sizes": sz, "tet_new": tet_new, "int_face_nitem": fn_.value, "int_node_nitem": nn_.value,
            "groups": groups, "seconds": seconds}


# ---- meshes and partitions ----------------------------------------------------------

def fix_empty(part, ngrp):
    """A copy of part in which every value 0..ngrp-1 occurs: tet g goes to an
    empty part g when its own part keeps another tet."""
    p = np.array(part, np.int32)
    cnt = np.bincount(p, minlength=ngrp)
    for g in np.nonzero(cnt == 0)[0]:
        k = next(k for k in range(len(p)) if cnt[p[k]] > 1)
        cnt[p[k]] -= 1
        p[k] = g
        cnt[g] += 1
    return p


def modulo_parts(ne, ngrp, seed=3):
    """part[k] = k % ngrp after a seeded permutation of the tets."""
    part = np.zeros(ne, np.int32)
    part[np.random.default_rng(seed).permutation(ne)] = np.arange(ne) % ngrp
    return part


def x_slabs(m, nparts):
    """nparts slabs along x with equal tet counts, from the centroids."""
    x = m.centroids()[:, 0]
    part = np.zeros(m.ne, np.int32)
    part[np.argsort(x, kind="stable")] = (np.arange(m.ne) * nparts) // m.ne
    return part


def glued_cubes():
    """Two kuhn_cube(2) blocks A and B that share one vertex only: B is A's
    copy translated by (1, 1, 1), its corner nearest (1, 1, 1) merged with A's
    corner nearest (1, 1, 1).  Returns (mesh, neA, the shared vertex)."""
    a = M.kuhn_cube(2, jitter=0.0)
    ca = int(np.argmin(((a.xyz[1:] - [1.0, 1.0, 1.0]) ** 2).sum(1))) + 1
    cb = int(np.argmin(((a.xyz[1:] - [0.0, 0.0, 0.0]) ** 2).sum(1))) + 1
    # B's vertices renumbered after A's, its corner cb mapped onto ca
    new = np.zeros(a.np + 1, np.int64)
    nxt = a.np
    for v in range(1, a.np + 1):
        if v == cb:
            new[v] = ca
        else:
            nxt += 1
            new[v] = nxt
    xyz = np.zeros((nxt + 1, 3))
    xyz[1:a.np + 1] = a.xyz[1:]
    keep = np.arange(1, a.np + 1) != cb
    xyz[new[1:][keep]] = a.xyz[1:][keep] + [1.0, 1.0, 1.0]
    tet = np.concatenate([a.tet, new[a.tet[1:]].astype(np.int32)]).astype(np.int32)
    return M.from_tets(xyz, tet), a.ne, ca


def glued_parts(m, ne_a, ids=(0, 2, 1)):
    """A in two slabs, the two sides of the plane x = y (it cuts no Kuhn tet and
    holds the corner (1, 1, 1), so both slabs touch it), with ids[0] and
    ids[1]; B whole with ids[2]."""
    c = m.centroids()
    part = np.full(m.ne, ids[2], np.int32)
    side = c[:ne_a, 0] < c[:ne_a, 1]
    part[:ne_a] = np.where(side, ids[0], ids[1])
    return part


def group_mesh(grp):
    """The Mesh of a fetched group (from_tets rebuilds adja and the trias)."""
    return M.from_tets(grp["xyz"], grp["tetra_v"])


def group_comm(grp, sp):
    """A split's group as the "old" communicators of a further split."""
    return {"face_index1": grp["face_index1"], "face_index2": grp["face_index2"],
            "node_index1": grp["node_index1"], "node_index2": grp["node_index2"],
            "int_face_nitem": sp["int_face_nitem"], "int_node_nitem": sp["int_node_nitem"]}


slabs = R.slabs
boustrophedon = R.boustrophedon
wave_mesh = R.wave_mesh
