"""The inputs of the location tests (no tests here): the smallest meshes and
point sets at which every branch of the location occurs, and their long-double
classifications (reference_locate), computed once per input and shared by the
CPU and the GPU module and by every run mode."""
from __future__ import annotations

import functools
import os

import numpy as np

import reference_locate as RL
from conftest import REF_INPUTS
from parmmg_amd import mesh as M
from test_gpu_edge_cases import delete_tets
from test_gpu_parity import _shuffled, l_shaped

VOLUME = ("lshape", "wave", "ties", "deleted", "shuffled")
SURFACE = ("cube6", "lshape6", "wave", "ridge", "cube6_h002", "ridge_h002")
CUBES = ("lshape", "ties", "deleted", "shuffled", "newpts6")     # jittered Kuhn meshes: ties are canonical


@functools.lru_cache(maxsize=None)
def _wave():
    return M.read_medit(os.path.join(REF_INPUTS, "wave.0.mesh"))


def tie_points(m, count=60):
    """The tie suite of test_tie_points_canonical: old vertices, edge
    midpoints, face centroids and centroids of `count` tets."""
    ks = np.random.default_rng(2).choice(np.arange(1, m.ne + 1), count, replace=False)
    P = m.xyz[m.tet[ks]]
    return np.concatenate([P[:, 0], 0.5 * (P[:, 0] + P[:, 1]), P[:, :3].mean(1), P.mean(1)])


def _unit_normals(m, ks):
    P = m.xyz[m.tria[ks]]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    return P, nrm / np.linalg.norm(nrm, axis=1)[:, None]


def surface_points(m, n=1200, seed=8):
    """n Dirichlet(0.6) combinations on random trias, 30 % of them pushed up
    to 50 % past an edge of their tria, each moved up to 1.5 hausd along the
    normal; then every 7th tria's first vertex and every 5th tria's first
    edge midpoint."""
    rng = np.random.default_rng(seed)
    ks = rng.integers(1, m.nt + 1, n)
    w = rng.dirichlet([0.6] * 3, n)
    push = np.nonzero(rng.random(n) < 0.3)[0]
    l = rng.integers(0, 3, len(push))
    over = rng.uniform(0.0, 0.5, len(push))
    rest = 1.0 - w[push, l]
    w[push] *= ((1.0 + over) / rest)[:, None]
    w[push, l] = -over
    P, nrm = _unit_normals(m, ks)
    x = np.einsum("nk,nkd->nd", w, P) + (rng.uniform(-1.5, 1.5, n) * m.hausd)[:, None] * nrm
    verts = m.xyz[m.tria[1::7, 0]]
    mids = 0.5 * (m.xyz[m.tria[1::5, 0]] + m.xyz[m.tria[1::5, 1]])
    return np.ascontiguousarray(np.concatenate([x, verts, mids]))


def ridge_points(m, seed=33):
    """Points outside the unit cube next to its ridges, where only the shadow
    wedge and the cone accept: the 8 corners moved outward along the three
    axes (6 draws each), the other vertices on the 12 cube edges moved outward
    along their two axes (2 draws each), and 2 random points on every
    boundary-tria edge that lies on a cube edge, moved outward likewise."""
    rng = np.random.default_rng(seed)
    X = m.xyz
    onb = (X == 0.0) | (X == 1.0)
    onb[0] = False
    out = np.where(X == 1.0, 1.0, -1.0) * onb                  # outward direction per boundary axis
    pts = []
    for ip in np.nonzero(onb.sum(1) == 3)[0]:
        for _ in range(6):
            pts.append(X[ip] + out[ip] * rng.uniform(0.1, 0.55, 3) * m.hausd)
    for ip in np.nonzero(onb.sum(1) == 2)[0]:
        for _ in range(2):
            pts.append(X[ip] + out[ip] * rng.uniform(0.1, 0.55, 3) * m.hausd)
    tr = m.tria[1:]
    e = np.concatenate([tr[:, [0, 1]], tr[:, [1, 2]], tr[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    e = e[(onb[e[:, 0]] & onb[e[:, 1]] & (X[e[:, 0]] == X[e[:, 1]])).sum(1) == 2]
    for a, b in e:
        for _ in range(2):
            s = rng.uniform(0.05, 0.95)
            both = onb[a] & onb[b]
            pts.append(X[a] + s * (X[b] - X[a]) + out[a] * both * rng.uniform(0.1, 0.6, 3) * m.hausd)
    return np.ascontiguousarray(np.array(pts))


@functools.lru_cache(maxsize=None)
def volume_case(name):
    """(mesh, points (n, 3)) of a volume input."""
    if name in ("lshape", "deleted", "shuffled"):
        m = l_shaped(8)
        x = np.random.default_rng(7).uniform(-0.1, 1.1, size=(600, 3))
        if name == "shuffled":
            m = _shuffled(m)
            x = np.concatenate([x, tie_points(m, 20)])          # min C under another numbering
        if name == "deleted":
            c = m.centroids()
            hole = 1 + np.nonzero(np.linalg.norm(c - np.array([0.3, 0.45, 0.4]), axis=1) < 0.17)[0]
            hole = hole[hole > 1]
            w = np.random.default_rng(13).dirichlet(np.ones(4), len(hole[::3]))      # strictly inside deleted tets
            x = np.concatenate([x, np.einsum("nk,nkd->nd", w, m.xyz[m.tet[hole[::3]]])])
            m = delete_tets(m, hole)
        return m, x
    if name == "wave":
        m = _wave()
        lo, hi = m.xyz[1:].min(0), m.xyz[1:].max(0)
        g = 0.05 * (hi - lo)
        return m, np.random.default_rng(11).uniform(lo - g, hi + g, size=(300, 3))
    if name == "ties":
        m = M.kuhn_cube(4)
        return m, tie_points(m)
    if name == "newpts6":
        m = M.kuhn_cube(6)
        x, t = M.new_points(6)
        return m, np.ascontiguousarray(x[t == 0])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def surface_case(name):
    """(mesh, points (n, 3)) of a surface input."""
    if name == "cube6":
        m = M.kuhn_cube(6)
        return m, surface_points(m, seed=8)
    if name == "lshape6":
        m = l_shaped(6)
        return m, surface_points(m, seed=8)
    if name == "wave":
        m = _wave()
        return m, surface_points(m, seed=6)
    if name == "wave_skip":                       # holds one cone answer through the reference's flag skip
        m = _wave()
        return m, surface_points(m, seed=4)
    if name == "ridge":
        m = M.kuhn_cube(6)
        return m, ridge_points(m)
    if name in ("cube6_h002", "ridge_h002"):
        m, x = surface_case(name[:-5])
        return M.from_tets(m.xyz, m.tet, hausd=0.002), x
    if name == "newpts6":
        m = M.kuhn_cube(6)
        x, t = M.new_points(6)
        return m, np.ascontiguousarray(x[t != 0])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def volume_reference(name):
    return RL.volume_ref(*volume_case(name))


@functools.lru_cache(maxsize=None)
def surface_reference(name):
    return RL.surface_ref(*surface_case(name))


def holes(name):
    """The deleted tets of a volume input."""
    m, _ = volume_case(name)
    return np.nonzero(m.tet[1:, 0] <= 0)[0] + 1


# The least number of answers per class an input must give (oracle and device):
# about 80 % of what the oracle gave when the inputs were written, so that an
# input that drifts cannot empty a branch; the ridge set must give at least 200
# wedge and 40 cone answers.
VOLUME_MIN = {
    "lshape": dict(found=250, not_found=250),
    "wave": dict(found=80, not_found=150),
    "ties": dict(found=240, ties=150),
    "deleted": dict(found=240, not_found=270),
    "shuffled": dict(found=330, not_found=250, ties=50),
}
SURFACE_MIN = {
    "cube6": dict(inside=600, border_edge=60, border_vertex=50, wedge=4, not_found=300),
    "lshape6": dict(inside=600, border_edge=60, border_vertex=50, wedge=4, not_found=300),
    "wave": dict(inside=500, border_edge=130, border_vertex=95, wedge=20, cone=1, not_found=300),
    "ridge": dict(wedge=200, cone=40),
    "cube6_h002": dict(inside=120, border_edge=60, border_vertex=50, not_found=900),
    "ridge_h002": dict(not_found=280),
}
# ... and of the path classes the oracle's walk from tria 1 reaches (the device
# starts next to the point: it is held to the oracle's own count from its starts)
SURFACE_MIN_ORACLE = {"lshape6": dict(exhaustive=8), "wave": dict(exhaustive=150)}


def assert_min_counts(rep, mins, what):
    for cls, least in mins.items():
        assert rep[cls] >= least, (what, cls, rep[cls], least)
