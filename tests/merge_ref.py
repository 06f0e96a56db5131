"""The CPU twin of pmx_merge_groups / pmx_merge_fetch / pmx_merge_maps
(tests/c/merge_ref.c) through ctypes, and the cases the merge tests share (test
infrastructure).  The twin is UNPINNED: Mmg is absent, so the reference file it
restates (src/mergemesh_pmmg.c) cannot be built here; tests/test_merge_cpu.py
checks it by properties instead.

Groups are the dicts Transfer.split_fetch and split_ref.split return; comm is
{"int_node_nitem", "int_face_nitem", "ext_node": [arrays], "ext_face": [arrays]}."""
import ctypes as C
import os
import subprocess
import time

import numpy as np

import split_ref as S
from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "merge_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libmerge_ref.so")

INT_KEYS = ("tetra_v", "tet_group", "tet_old", "point_group", "point_old", "node_index1", "node_index2",
            "face_index1", "face_index2", "ext_node_items", "ext_face_items")
OUT_KEYS = ("tetra_v", "tet_group", "tet_old", "point_group", "point_old", "point_new", "tet_new", "node_index1",
            "node_index2", "face_index1", "face_index2", "ext_node_items", "ext_face_items")
SENT = -77

_lib = None


class Sizes(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("np", "ne", "nnode", "nface")]


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
        l.mgr_merge.restype = C.c_int
        l.mgr_merge.argtypes = [C.c_int] + [vp] * 9 + [C.c_int, vp, i64, i64, C.c_int, vp, vp, C.c_int, vp, vp] + \
                               [vp] * 14
        l.mgr_last_error.restype = C.c_char_p
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def pack(groups, comm=None):
    """The flat arrays the twin takes, as a dict (the refusal tests edit it)."""
    comm = comm or {}
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    cat = lambda arrs: i32(np.concatenate(arrs)) if arrs else np.zeros(0, np.int32)
    off = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    key = lambda k: [i32(g.get(k, np.zeros(0))).ravel() for g in groups]
    f = {"ngrp": len(groups),
         "poff": off([g["xyz"].shape[0] - 1 for g in groups]), "toff": off([g["tetra_v"].shape[0] - 1 for g in groups]),
         "noff": off([len(g.get("node_index1", ())) for g in groups]),
         "foff": off([len(g.get("face_index1", ())) for g in groups]),
         "tet": cat([i32(g["tetra_v"])[1:].ravel() for g in groups]),
         "node1": cat(key("node_index1")), "node2": cat(key("node_index2")),
         "face1": cat(key("face_index1")), "face2": cat(key("face_index2")),
         "nsol": len(groups[0]["sols"]) if groups else 0,
         "sol_size": i32([s.shape[1] for g in groups for s in g["sols"]]),
         "nitem_node": int(comm.get("int_node_nitem", 0)), "nitem_face": int(comm.get("int_face_nitem", 0))}
    for kind in ("node", "face"):
        lists = [i32(a) for a in comm.get("ext_" + kind, [])]
        f["next_" + kind] = len(lists)
        f[kind + "_off"] = off([len(a) for a in lists])
        f[kind + "_items"] = cat(lists)
    return f


def outputs(f, fill=0):
    """Output arrays large enough for any result of the packed input f."""
    P, T = int(f["poff"][-1]), int(f["toff"][-1])
    nen, nef = len(f["node_items"]), len(f["face_items"])
    n = {"tetra_v": 4 * T, "tet_group": T, "tet_old": T, "point_group": P, "point_old": P, "point_new": P,
         "tet_new": T, "node_index1": nen, "node_index2": nen, "face_index1": nef, "face_index2": nef,
         "ext_node_items": nen, "ext_face_items": nef}
    return {k: np.full(max(n[k], 1), fill, np.int32) for k in OUT_KEYS}


def call(f, out, sizes=None):
    """mgr_merge on packed input f into the arrays out: (return value, sizes, error, seconds)."""
    sz = sizes if sizes is not None else Sizes()
    t0 = time.perf_counter()
    r = lib().mgr_merge(f["ngrp"], _p(f["poff"]), _p(f["toff"]), _p(f["noff"]), _p(f["foff"]), _p(f["tet"]),
                        _p(f["node1"]), _p(f["node2"]), _p(f["face1"]), _p(f["face2"]), f["nsol"], _p(f["sol_size"]),
                        f["nitem_node"], f["nitem_face"], f["next_node"], _p(f["node_off"]), _p(f["node_items"]),
                        f["next_face"], _p(f["face_off"]), _p(f["face_items"]), C.byref(sz),
                        *[_p(out[k]) for k in OUT_KEYS])
    return r, sz, lib().mgr_last_error().decode(), time.perf_counter() - t0


def merge(groups, comm=None):
    """The merge of groups: a dict with sizes ((4,) int64: np, ne, nnode, nface),
    the arrays Transfer.merge_fetch returns (xyz and sols gathered from the
    creating copies) and maps, a list of (point_new, tet_new) per group;
    seconds: the C call alone.  RuntimeError on a refusal."""
    f = pack(groups, comm)
    out = outputs(f)
    r, sz, err, seconds = call(f, out)
    if not r:
        raise RuntimeError("mgr_merge: " + err)
    npm, nem, nn, nf = sz.np, sz.ne, sz.nnode, sz.nface
    d = {"sizes": np.array([npm, nem, nn, nf], np.int64), "seconds": seconds}
    tv = np.zeros((nem + 1, 4), np.int32)
    tv[1:] = out["tetra_v"][:4 * nem].reshape(nem, 4)
    d["tetra_v"] = tv
    for k, n in (("tet_group", nem), ("tet_old", nem), ("point_group", npm), ("point_old", npm), ("node_index1", nn),
                 ("node_index2", nn), ("face_index1", nf), ("face_index2", nf),
                 ("ext_node_items", len(f["node_items"])), ("ext_face_items", len(f["face_items"]))):
        d[k] = out[k][:n].copy()
    d["maps"] = [(out["point_new"][f["poff"][g]:f["poff"][g + 1]].copy(),
                  out["tet_new"][f["toff"][g]:f["toff"][g + 1]].copy()) for g in range(len(groups))]
    # rows of the creating copies
    d["xyz"] = np.zeros((npm + 1, 3))
    d["sols"] = [np.zeros((npm + 1, s.shape[1])) for s in groups[0]["sols"]]
    for g, grp in enumerate(groups):
        at = np.nonzero(d["point_group"] == g)[0]
        d["xyz"][at + 1] = grp["xyz"][d["point_old"][at]]
        for a, s in zip(d["sols"], grp["sols"]):
            a[at + 1] = s[d["point_old"][at]]
    return d


# ---- cases ------------------------------------------------------------------------------

def sols_of(m):
    return [M.on_vertices(m, M.iso_metric), M.on_vertices(m, M.velocity)]


def split_case(m, part, ngrp, sols=None):
    """m split by part with the twin of the split: (split dict, comm without
    external communicators)."""
    sols = sols if sols is not None else [np.ones((m.np + 1, 1))]
    sp = S.split(m, part, ngrp, data=(m.xyz, sols))
    return sp, {"int_node_nitem": sp["int_node_nitem"], "int_face_nitem": sp["int_face_nitem"]}


def remote_case(m, part, pieces=1, sols=None):
    """m split in three; groups 0 and 1 stay, group 2 plays another rank: the
    positions its lists share with the two others, ascending, in `pieces`
    external communicators each.  Returns (split, groups, comm, remote group)."""
    sp, comm = split_case(m, part, 3, sols)
    g0, g1, g2 = sp["groups"]
    chunks = lambda a: [c.astype(np.int32) for c in np.array_split(a, pieces)]
    for kind in ("node", "face"):
        mine = np.concatenate([g0[kind + "_index2"], g1[kind + "_index2"]])
        shared = np.intersect1d(g2[kind + "_index2"], mine)
        comm["ext_" + kind] = chunks(shared)
    return sp, [g0, g1], comm, g2


def cases():
    """name -> (mesh, part, ngrp, sols or None): the round-trip cases."""
    k3, k6 = M.kuhn_cube(3), M.kuhn_cube(6)
    out = {"k3_slabs2": (k3, S.slabs(k3, 2), 2, sols_of(k3)), "k3_slabs3": (k3, S.slabs(k3, 3), 3, sols_of(k3)),
           "k6_slabs8": (k6, S.slabs(k6, 8), 8, sols_of(k6)),
           "k6_boustrophedon": (k6, S.boustrophedon(k6, 6), 2, None),
           "k6_random5": (k6, S.fix_empty(np.random.default_rng(7).integers(0, 5, k6.ne), 5), 5, None),
           "k6_thousand": (k6, S.modulo_parts(k6.ne, 1000), 1000, None)}
    ms, tinv = M.numbering(k6, "shuffle")
    p = np.zeros(ms.ne, np.int32)
    p[tinv[1:] - 1] = S.slabs(k6, 8)
    out["k6_slabs8_shuffle"] = (ms, p, 8, sols_of(ms))
    w = S.wave_mesh()
    out["wave_xslabs4"] = (w, S.x_slabs(w, 4), 4, sols_of(w))
    gm, ne_a, _ = S.glued_cubes()
    out["glued"] = (gm, S.glued_parts(gm, ne_a), 3, None)
    return out
