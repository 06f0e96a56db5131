"""The CPU twin of pmx_moveifc_* (tests/c/moveifc_ref.c) through ctypes, and
the cases the interface-displacement tests share (test infrastructure).  The
twin is UNPINNED: Mmg is absent, so the reference file it restates cannot be
built here."""
import ctypes as C
import os
import subprocess

import numpy as np

import contiguity_ref as R
from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "moveifc_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libmoveifc_ref.so")
LMAX = 10240

_lib = None


class Map(C.Structure):
    _fields_ = [("nprocs", C.c_int), ("myrank", C.c_int), ("nold_grp", C.c_int),
                ("displsgrp", C.c_void_p), ("mapgrp", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("front", "touched", "recolor", "next", "blocks", "maxball", "overflow_ip")]


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
        vp, i64, mp = C.c_void_p, C.c_int64, C.POINTER(Map)
        l.mir_begin.restype = i64
        l.mir_begin.argtypes = [i64, i64, vp, mp, vp, vp, vp, vp, vp, vp, vp]
        l.mir_set_colors.restype = None
        l.mir_set_colors.argtypes = [i64, vp, vp, vp, vp]
        l.mir_layer.restype = C.c_int
        l.mir_layer.argtypes = [i64, i64, vp, vp, mp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        l.mir_part.restype = C.c_int
        l.mir_part.argtypes = [i64, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(C.c_int)]
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def single_map(weights):
    """One rank: the map of len(weights) old groups."""
    w = np.asarray(weights, np.int32)
    return {"nprocs": 1, "myrank": 0, "displsgrp": np.array([0, len(w)], np.int32), "mapgrp": w}


def counts(part, ngrp):
    return np.bincount(np.asarray(part), minlength=ngrp).astype(np.int32)


class Twin:
    """The sequential displacement of mesh m: begin on construction, then
    set_colors / layer; the state as numpy arrays (mark (ne,), tmp, s, front
    (np,) each, negrp, nemin)."""

    def __init__(self, m, tet_group, map):
        self.m = m
        self.ne, self.np = m.ne, m.np
        self.tet = np.ascontiguousarray(m.tet, np.int32)
        self.adja = np.ascontiguousarray(m.adja, np.int32)
        self.nprocs, self.myrank = int(map.get("nprocs", 1)), int(map.get("myrank", 0))
        self.displs = np.ascontiguousarray(map["displsgrp"], np.int32)
        self.mapgrp = np.ascontiguousarray(map["mapgrp"], np.int32)
        self.nold = int(self.displs[self.myrank + 1] - self.displs[self.myrank])
        self.cmap = Map(self.nprocs, self.myrank, self.nold, _p(self.displs), _p(self.mapgrp))
        self._mark = np.zeros(self.ne + 1, np.int32)
        self._tmp, self._s, self._flag = (np.zeros(self.np + 1, np.int32) for _ in range(3))
        self.negrp, self.nemin = np.zeros(self.nold, np.int32), np.zeros(self.nold, np.int32)
        tg = np.ascontiguousarray(tet_group, np.int32)
        self.nfront = int(lib().mir_begin(self.ne, self.np, _p(self.tet), C.byref(self.cmap), _p(tg), _p(self._mark),
                                          _p(self._tmp), _p(self._s), _p(self._flag), _p(self.negrp), _p(self.nemin)))

    mark = property(lambda self: self._mark[1:])
    tmp = property(lambda self: self._tmp[1:])
    s = property(lambda self: self._s[1:])
    front = property(lambda self: self._flag[1:])

    def weight(self, color):
        c = np.asarray(color)
        return self.mapgrp[c // self.nprocs + self.displs[c % self.nprocs]]

    def colors(self, ip):
        return self._tmp[np.asarray(ip)].copy()

    def set_colors(self, ip, color):
        ip, color = np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(color, np.int32)
        lib().mir_set_colors(len(ip), _p(ip), _p(color), _p(self._tmp), _p(self._flag))

    def layer(self):
        """(ok, stats dict); blocked = blocks > 0."""
        st = Stats()
        ok = lib().mir_layer(self.ne, self.np, _p(self.tet), _p(self.adja), C.byref(self.cmap), _p(self._mark),
                             _p(self._tmp), _p(self._s), _p(self._flag), _p(self.negrp), _p(self.nemin), C.byref(st))
        d = {f: getattr(st, f) for f, _ in st._fields_}
        d["blocked"] = int(d["blocks"] > 0)
        return bool(ok), d

    def snapshot(self):
        return {k: getattr(self, k).copy() for k in ("mark", "tmp", "s", "front", "negrp", "nemin")}

    def part(self, target, ngrps_all=None, mark=None):
        """(ok, part, ngrp) of PMMG_part_getInterfaces on mark (default: own)."""
        mk = self._mark if mark is None else np.concatenate([[0], np.asarray(mark, np.int32)]).astype(np.int32)
        ng = np.ascontiguousarray(np.diff(self.displs) if ngrps_all is None else ngrps_all, np.int32)
        part = np.zeros(self.ne, np.int32)
        n = C.c_int(0)
        ok = lib().mir_part(self.ne, _p(mk), self.nprocs, self.myrank, self.nold, target, _p(ng), _p(part), C.byref(n))
        return bool(ok), part, n.value


# ---- meshes -------------------------------------------------------------------------

def two_cubes_corner(n=2):
    """Two Kuhn cubes that share one corner vertex only: the ball of that
    vertex has two face-connected components."""
    a = M.kuhn_cube(n)
    b = M.kuhn_cube(n)
    corner_a = int(np.argmin(((a.xyz[1:] - [1.0, 1.0, 1.0]) ** 2).sum(1))) + 1
    corner_b = int(np.argmin(((b.xyz[1:] - [0.0, 0.0, 0.0]) ** 2).sum(1))) + 1
    # b's points renumbered after a's, its corner identified with a's
    new = np.zeros(b.np + 1, np.int64)
    nxt = a.np + 1
    for p in range(1, b.np + 1):
        if p == corner_b:
            new[p] = corner_a
        else:
            new[p] = nxt
            nxt += 1
    keep = np.array([p for p in range(1, b.np + 1) if p != corner_b])
    xyz = np.concatenate([a.xyz, b.xyz[keep] + [1.0, 1.0, 1.0]])
    tet = np.concatenate([a.tet, new[b.tet[1:]]]).astype(np.int32)
    return M.from_tets(xyz, tet), a.ne, corner_a


def cone(g):
    """An apex over a g x g square of 2 g^2 triangles: 2 g^2 tets, all in the
    apex's ball.  Returns (mesh, apex)."""
    n1 = g + 1
    xs, ys = np.meshgrid(np.arange(n1) / g, np.arange(n1) / g, indexing="ij")
    base = np.stack([xs.ravel(), ys.ravel(), np.zeros(n1 * n1)], 1)
    xyz = np.concatenate([[[0.0, 0.0, 0.0]], base, [[0.5, 0.5, 1.0]]])
    apex = n1 * n1 + 1
    idx = lambda i, j: 1 + i * n1 + j
    tets = [[0, 0, 0, 0]]
    for i in range(g):
        for j in range(g):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tets.append([a, b, c, apex])
            tets.append([a, c, d, apex])
    return M.from_tets(xyz, np.array(tets, np.int32)), apex


# ---- the cases (shared by the CPU and the GPU tests) -----------------------------------

def _cube(n, f):
    m = M.kuhn_cube(n)
    x, y, z = R.cells(m, n).T
    return m, f(x, y, z).astype(np.int32)


def build(name):
    """(mesh, tet_group, map, nlayers, node (points, exchange weights) or None)."""
    shuffle = name.endswith("@shuffle")
    base = name[:-8] if shuffle else name
    node = None
    if base == "empty_slabs":
        m, tg = _cube(6, lambda x, y, z: (z >= 1) * 1 + (z >= 3))
        mp, nl = single_map(counts(tg, 3)), 2
    elif base == "equal_slabs":
        m, tg = _cube(6, lambda x, y, z: z // 2)
        mp, nl = single_map(counts(tg, 3)), 2
    elif base == "revquad":
        m, tg = _cube(6, lambda x, y, z: (x >= 4) + 2 * (y >= 3))
        mp, nl = single_map(counts(tg, 4)), 3
    elif base == "octants":
        m, tg = _cube(6, lambda x, y, z: (x >= 4) + 2 * (y >= 3) + 4 * (z >= 2))
        mp, nl = single_map(counts(tg, 8)), 3
    elif base == "ties":
        m, tg = _cube(6, lambda x, y, z: (x >= 3) + 2 * (y >= 3))
        mp, nl = single_map([900, 500, 500, 200]), 4
    elif base.startswith("frag_"):                      # frag_<n>_<big|counts>
        _, n, kind = base.split("_")
        m = M.kuhn_cube(int(n))
        tg = np.random.default_rng(1 if kind == "big" else 2).integers(0, 5, m.ne).astype(np.int32)
        mp = single_map([100000, 100001, 100000, 99999, 100002] if kind == "big" else counts(tg, 5))
        nl = 3
    elif base == "revslabs":
        m, tg = _cube(6, lambda x, y, z: (z >= 3) * 1 + (z >= 5))
        mp, nl = single_map(counts(tg, 3)), 2
    elif base == "tiny":
        m = M.kuhn_cube(6)
        tg = R.slabs(m, 2).astype(np.int32)
        R.plant(m, tg, [R.nearest(m, 0.5, 0.5, 0.8)], 2, 8)
        R.plant(m, tg, [R.nearest(m, 0.2, 0.2, 0.2)], 3, 1)
        R.plant(m, tg, [R.nearest(m, 0.8, 0.3, 0.3)], 4, 2)
        mp, nl = single_map(counts(tg, 5)), 5
    elif base == "wave_bisect":
        m = R.wave_mesh()
        c = m.centroids()
        tg = (2 * (c[:, 0] < np.median(c[:, 0])) + (c[:, 1] < np.median(c[:, 1]))).astype(np.int32)
        # the lighter colours later in tet order
        order = np.argsort([np.nonzero(tg == g)[0].mean() for g in range(4)])
        w = np.zeros(4, np.int32)
        w[order] = [4000, 3000, 2000, 1000]
        mp, nl = single_map(w), 2
    elif base == "wave_random":
        m = R.wave_mesh()
        tg = np.random.default_rng(11).integers(0, 4, m.ne).astype(np.int32)
        mp, nl = single_map([500000, 500003, 499999, 500001]), 2
    elif base in ("ranks3", "ranks3_big"):
        # nprocs = 3, myrank = 1: own colours 1, 4, 7; the points of the face
        # x = 0 are the node communicator, fed foreign colours 0, 2, 5.
        # ranks3: the own weights are the tet counts, so layers block;
        # ranks3_big: weights that are no counts, so that negrp never nears
        # nemin and foreign colours meet the parallel path -- colour 0 (4500)
        # beats the own colour 1 (5000) and is beaten by 4 (4000), 7 (3000)
        # and 2 (2000): tets are recoloured to and from foreign colours
        m, tg = _cube(6, lambda x, y, z: z // 2)
        displs = np.array([0, 1, 4, 6], np.int32)                # rank 0: 1 group, rank 1: 3, rank 2: 2
        mapgrp = np.array([300, 432, 430, 434, 10, 600] if base == "ranks3"
                          else [4500, 5000, 4000, 3000, 2000, 6000], np.int32)   # colours 0 | 1 4 7 | 2 5
        mp, nl = {"nprocs": 3, "myrank": 1, "displsgrp": displs, "mapgrp": mapgrp}, 3
        pts = (np.nonzero(m.xyz[1:, 0] == 0.0)[0] + 1).astype(np.int32)
        node = (pts, np.array([0, 2, 5], np.int32))
    elif base == "corner":
        m, ne_a, corner = two_cubes_corner(2)
        tg = np.zeros(m.ne, np.int32)
        tg[ne_a:] = 1                       # the second cube, lighter and later
        tg[:ne_a // 2] = 2                  # and a heavier colour in the first
        mp, nl = single_map([1000, 10, 2000]), 2
    elif base.startswith("cone_"):
        m, apex = cone(int(base[5:]))
        tg = np.zeros(m.ne, np.int32)
        tg[m.ne // 2:] = 1                  # the lighter colour later
        mp, nl = single_map([3 * m.ne, m.ne]), 1
    else:
        raise KeyError(name)
    if shuffle:
        m2, tinv = M.numbering(m, "shuffle")
        tg2 = np.zeros_like(tg)
        tg2[tinv[1:] - 1] = tg              # tet_group follows the tets
        if node is not None:
            raise KeyError("no shuffled multi-rank case")
        m, tg = m2, tg2
    return m, tg, mp, nl, node


def exchange_fn(twin_weight, node, layer):
    """The emulated exchange of case ranks3: every third listed point is
    offered a foreign colour, which it takes when that beats its own."""
    pts, foreign = node

    def f(colors):
        out = np.array(colors, np.int32)
        for i in range(len(out)):
            if (i + layer) % 3 == 0:
                c = foreign[(i // 3 + layer) % len(foreign)]
                if twin_weight(c) < twin_weight(out[i]):
                    out[i] = c
        return out
    return f


_runs = {}


def run(name):
    """The twin's run of a case, computed once: (mesh, tet_group, map, node,
    begin snapshot + nfront, [(ok, stats, snapshot) per layer])."""
    if name not in _runs:
        m, tg, mp, nl, node = build(name)
        t = Twin(m, tg, mp)
        begin = t.snapshot()
        begin["nfront"] = t.nfront
        layers, t.pres = [], []                             # t.pres: each layer's start, after its exchange
        for l in range(nl):
            if node is not None:
                t.set_colors(node[0], exchange_fn(t.weight, node, l)(t.colors(node[0])))
            pre = t.snapshot()
            t.pres.append(pre)
            ok, st = t.layer()
            layers.append((ok, st, t.snapshot() if ok else pre))
            if not ok:
                break
        _runs[name] = (m, tg, mp, node, begin, layers, t)
    return _runs[name]


# ---- the parallel formulation, restated ----------------------------

INXT3 = [1, 2, 3, 0, 1, 2, 3]


def ball(m, slot):
    """The slots 4 k + j of the ball of the vertex at `slot`, breadth-first
    through the three faces that hold it, in the order inxt3."""
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) // 4
    p = m.tet[slot // 4, slot % 4]
    lst, seen, cur = [slot], {slot // 4}, 0
    while cur < len(lst):
        k, i = lst[cur] // 4, lst[cur] % 4
        for _ in range(3):
            i = INXT3[i]
            k1 = int(nb[k - 1, i])
            if k1 and k1 not in seen:
                seen.add(k1)
                lst.append(4 * k1 + list(m.tet[k1]).index(p))
        cur += 1
    return lst


def model_layer(m, t, pre):
    """The parallel formulation on the state `pre`, in Python, independent of
    the twin's loops: (post state, D, recolourings, touched points, balls, the
    recolourings whose previous colour was foreign)."""
    w = lambda c: int(t.weight(np.asarray(c)))
    mark = np.concatenate([[0], pre["mark"]])
    tmp = np.concatenate([[0], pre["tmp"]])
    s = np.concatenate([[0], pre["s"]])
    flag = np.concatenate([[0], pre["front"]])
    fronts = [p for p in range(1, m.np + 1) if flag[p] and s[p] >= 0]
    balls = {p: ball(m, int(s[p])) for p in fronts}
    reach = {}                                           # tet -> [(ip, j, pos)]
    for p in fronts:
        for pos, sl in enumerate(balls[p]):
            reach.setdefault(sl // 4, []).append((p, sl % 4, pos))
    new = mark.copy()
    D = np.zeros(len(pre["negrp"]), np.int64)
    nrec, nforeign, best = 0, 0, {}                      # q -> (weight, ip, pos, slot)
    for k, lst in reach.items():
        cur = int(mark[k])
        for ip, j, pos in sorted(lst):
            c = int(tmp[ip])
            if not w(c) < w(cur):
                continue
            nrec += 1
            if cur % t.nprocs == t.myrank:
                D[cur // t.nprocs] += 1
            else:
                nforeign += 1
            for a in range(3):
                j2 = INXT3[j + a]
                q = int(m.tet[k, j2])
                ev = (w(c), ip, pos, 4 * k + j2)
                if q not in best or ev[:3] < best[q][:3]:
                    best[q] = ev
            cur = c
        new[k] = cur
    tmp2, s2, flag2 = tmp.copy(), s.copy(), np.zeros_like(flag)
    touched = []
    for q, (wq, ip, pos, slot) in best.items():
        if flag[q]:
            touched.append(q)
        elif wq < w(tmp[q]):
            tmp2[q], s2[q] = tmp[ip], slot
        flag2[q] = 1
    for q in touched:                                    # the side fronts on the final marks
        for sl in balls[q]:
            if w(new[sl // 4]) < w(tmp2[q]):
                tmp2[q], s2[q] = new[sl // 4], sl
    post = {"mark": new[1:], "tmp": tmp2[1:], "s": s2[1:], "front": flag2[1:], "negrp": pre["negrp"] - D}
    return post, D, nrec, len(touched), balls, nforeign


PARALLEL_CASES = ["revquad", "octants", "ties", "frag_4_big", "frag_6_big"]
SHUFFLED_PARALLEL = [c + "@shuffle" for c in ("revquad", "octants", "frag_4_big", "frag_6_big")]
SHUFFLED_BLOCKING = ["frag_4_counts@shuffle", "frag_6_counts@shuffle"]
CASES = (["empty_slabs", "equal_slabs"] + PARALLEL_CASES + ["frag_4_counts", "frag_6_counts", "revslabs", "tiny"] +
         SHUFFLED_PARALLEL + SHUFFLED_BLOCKING + ["wave_bisect", "wave_random", "ranks3", "ranks3_big", "corner",
                                                  "cone_71"])
