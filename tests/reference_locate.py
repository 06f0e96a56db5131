"""A brute-force long-double definition of a correct point location (no tests here).

Plain numpy in ``np.longdouble``, every point against every element, written
from the definitions and not from the oracle: a tet's barycentric lambda_i is
the ratio of two 3x3 determinants (the tet with vertex i replaced by the point,
over the tet); a tria's are the signed area ratios of the point's orthogonal
projection on the tria's plane.  No stored face normals, no walk.

EPS = 1e-6 (MMG5_EPS).  A tet / tria k is valid when its first vertex is > 0.

Volume, per point p

* C(p) = the valid tets with min_i lambda_i > -EPS;
* d_k(p) = |min_i lambda_i| vol_k, vol the triple product; closest(p) = argmin_k d_k.

(elem, status) is correct iff status in {1, -1} and elem in C(p), or status == 0,
C(p) empty and elem == closest(p).  canonical: additionally elem == min C(p).

Surface, per point p and returned tria k: n the unit normal of k, h = (p - v0).n,
lambda the barycentrics of p - h n, T(p) = the valid trias with min lambda > -EPS
and |h| <= hausd.  Correct iff

* status 1, no edge, no vertex: k in T(p) and min lambda >= EPS;
* status 1, edge l, lambda_l > -EPS: k in T(p), lambda_l = min lambda < EPS, the
  second smallest >= EPS;
* status 1, edge l, lambda_l <= -EPS (shadow wedge): a = v_{l+2} - v_{l+1},
  alpha = a.(p - v_{l+1}), 0 <= alpha <= |a|^2 and p within hausd of the edge's line;
* status 1, vertex i: k in T(p) with the two smallest lambda < EPS and i = argmax
  lambda, or the cone: |p - x_ip| <= hausd and (x_j - x_ip).(p - x_ip) <= 0 for
  every vertex j != ip of every valid tria incident to ip = tria[k, i];
* status -1: k in T(p), no edge, no vertex;
* status 0: T(p) empty and k the valid tria whose centroid is nearest to p.

The cone as the reference runs it is not this predicate on every path:
PMMG_locatePointInCone flags a neighbour before it tests it and skips the
neighbours already flagged with the cone's vertex (src/locate_pmmg.c:248-249),
so a second cone test at the same vertex in one query no longer sees the
neighbour that rejected the first.  A vertex answer within hausd of its vertex
that fails the full predicate is therefore reported as class cone_skip, with
its point in `skipped`, and not as a violation: the tests require `skipped` to
be empty on the oracle's inputs and equal to the oracle's on the device.

Undecidable (left out of the assertions, counted): a tested quantity within
TOL = 1e-9 of its threshold (absolute for lambda, |h| - hausd and dist - hausd,
relative to |a|^2 for alpha and the cone's products), or the two smallest d_k /
centroid distances of a not-found point within 1e-9 relative.  A quantity that
equals its threshold exactly in long double is decided by the closed
inequality: the ridge inputs hold points exactly above the end of an
axis-aligned edge, where alpha is 0 or |a|^2 without rounding.
"""
from __future__ import annotations

import numpy as np
import pytest

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:            # no extended precision on this platform
    pytest.skip("np.longdouble is not wider than float64 here", allow_module_level=True)

EPS = LD(1e-6)
TOL = LD(1e-9)
PAIRS_BUDGET = 150_000       # (point, element) pairs evaluated at once


def _triple(a, b, c):
    """a . (b x c) over the last axis."""
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1])
            + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2])
            + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _det4(a, b, c, d):
    """The determinant of the tet (a, b, c, d): (b - a) . ((c - a) x (d - a))."""
    return _triple(b - a, c - a, d - a)


def tet_lambdas(P, p):
    """P (..., 4, 3) tets, p (..., 3) points (broadcast against each other) ->
    (lambda (..., 4), vol (...)): lambda_i = det(tet with vertex i := p) / det(tet)."""
    P, p = np.asarray(P, LD), np.asarray(p, LD)
    v = [P[..., i, :] for i in range(4)]
    vol = _det4(*v)
    lam = np.stack([_det4(*[p if j == i else v[j] for j in range(4)]) for i in range(4)], -1)
    return lam / vol[..., None], vol


def tria_lambdas(P, p):
    """P (..., 3, 3) trias, p (..., 3) -> (lambda (..., 3), h (...)): h the signed
    distance of p to the tria's plane, lambda_i the area of (q, v_{i+1}, v_{i+2})
    over the tria's, q = p - h n, both signed by the unit normal n."""
    P, p = np.asarray(P, LD), np.asarray(p, LD)
    v = [P[..., i, :] for i in range(3)]
    N = _cross(v[1] - v[0], v[2] - v[0])
    area = np.sqrt(_dot(N, N))
    n = N / area[..., None]
    h = _dot(p - v[0], n)
    q = p - h[..., None] * n
    lam = np.stack([_dot(_cross(v[(i + 1) % 3] - q, v[(i + 2) % 3] - q), n) for i in range(3)], -1)
    return lam / area[..., None], h


def _two_smallest(d, ids):
    """Per row of d (n, K): (id of the smallest, id of the second, tie flag)."""
    n, K = d.shape
    if K == 0:
        z = np.zeros(n, np.int64)
        return z, z, np.zeros(n, bool)
    o = np.argsort(d, axis=1, kind="stable")
    r = np.arange(n)
    a = o[:, 0]
    if K == 1:
        return ids[a], np.zeros(n, np.int64), np.zeros(n, bool)
    b = o[:, 1]
    da, db = d[r, a], d[r, b]
    return ids[a], ids[b], (db - da) <= TOL * db


def volume_ref(m, x):
    """The classification of the points x (n, 3) against every valid tet of m:
    inC (n, ne+1) bool, minC / nC (n,), closest / second (n,) by d_k, und (n,)."""
    x = np.asarray(x, np.float64)
    n, ne = len(x), m.ne
    ids = np.nonzero(m.tet[1:, 0] > 0)[0] + 1
    P = np.asarray(m.xyz[m.tet[ids]], LD)
    inC = np.zeros((n, ne + 1), bool)
    und = np.zeros(n, bool)
    closest, second, tie = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool))
    step = max(1, PAIRS_BUDGET // max(len(ids), 1))
    for a in range(0, n, step):
        p = np.asarray(x[a:a + step], LD)[:, None, :]
        lam, vol = tet_lambdas(P[None], p)
        lmin = lam.min(-1)
        inC[a:a + step, ids] = lmin > -EPS
        und[a:a + step] = (np.abs(lmin + EPS) <= TOL).any(1)
        closest[a:a + step], second[a:a + step], tie[a:a + step] = _two_smallest(np.abs(lmin) * vol, ids)
    nC = inC.sum(1)
    minC = np.where(nC > 0, np.argmax(inC, axis=1), 0)
    und |= (nC == 0) & tie
    return dict(n=n, valid=ids, inC=inC, nC=nC, minC=minC, closest=closest, second=second, und=und)


def surface_ref(m, x, hausd=None):
    """The classification of the points x (n, 3) against every valid tria of m:
    inT (n, nt+1) bool, nT (n,), nearest / second (n,) by the centroid distance,
    und (n,).  hausd: the mesh's unless given."""
    x = np.asarray(x, np.float64)
    hausd = LD(m.hausd if hausd is None else hausd)
    n, nt = len(x), m.nt
    ids = np.nonzero(m.tria[1:, 0] > 0)[0] + 1
    P = np.asarray(m.xyz[m.tria[ids]], LD)
    cen = (P[:, 0] + P[:, 1] + P[:, 2]) / 3
    inT = np.zeros((n, nt + 1), bool)
    und = np.zeros(n, bool)
    nearest, second, tie = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool))
    step = max(1, PAIRS_BUDGET // max(len(ids), 1))
    for a in range(0, n, step):
        p = np.asarray(x[a:a + step], LD)[:, None, :]
        lam, h = tria_lambdas(P[None], p)
        lmin, ah = lam.min(-1), np.abs(h)
        inT[a:a + step, ids] = (lmin > -EPS) & (ah <= hausd)
        und[a:a + step] = (((np.abs(lmin + EPS) <= TOL) & (ah <= hausd + TOL))
                           | ((np.abs(ah - hausd) <= TOL) & (lmin > -EPS - TOL))).any(1)
        r = p - cen[None]
        nearest[a:a + step], second[a:a + step], tie[a:a + step] = _two_smallest(np.sqrt(_dot(r, r)), ids)
    nT = inT.sum(1)
    und |= (nT == 0) & tie
    # the valid trias around every vertex, for the cone
    fan = {}
    for k in ids:
        for ip in m.tria[k]:
            fan.setdefault(int(ip), []).append(int(k))
    return dict(n=n, valid=ids, inT=inT, nT=nT, nearest=nearest, second=second, und=und, hausd=hausd, fan=fan)


def _report(classes):
    rep = {c: 0 for c in classes}
    rep["violations"] = []
    rep["undecidable"] = 0
    return rep


def summary(rep):
    """The report's counts (its lists by their length)."""
    return {k: (len(v) if isinstance(v, list) else v) for k, v in rep.items()}


def check_volume(m, x, elem, status, canonical: bool, ref=None):
    """The report of the volume answers (elem, status) of the points x: counts
    per class (found, exhaustive, not_found, ties = found with |C| > 1,
    undecidable) and the violations [(point, reason)] on decidable points."""
    ref = volume_ref(m, x) if ref is None else ref
    assert ref["n"] == len(x) == len(elem) == len(status)
    rep = _report(("found", "exhaustive", "not_found", "ties"))
    inC, nC = ref["inC"], ref["nC"]
    for i in range(len(x)):
        if ref["und"][i]:
            rep["undecidable"] += 1
            continue
        k, s = int(elem[i]), int(status[i])
        bad = None
        if not (1 <= k <= m.ne and m.tet[k, 0] > 0):
            bad = f"tet {k} is not a valid tet"
        elif s in (1, -1):
            rep["found" if s == 1 else "exhaustive"] += 1
            rep["ties"] += int(nC[i] > 1)
            if not inC[i, k]:
                bad = f"status {s} but tet {k} does not hold the point" + (
                    f" (C is empty, closest {ref['closest'][i]})" if nC[i] == 0 else f" (min C {ref['minC'][i]})")
            elif canonical and k != ref["minC"][i]:
                bad = f"tet {k} holds the point but min C is {ref['minC'][i]}"
        elif s == 0:
            rep["not_found"] += 1
            if nC[i] > 0:
                bad = f"status 0 but {nC[i]} tets hold the point (min C {ref['minC'][i]})"
            elif k != ref["closest"][i]:
                bad = f"status 0 with tet {k}, the closest is {ref['closest'][i]}"
        else:
            bad = f"status {s}"
        if bad:
            rep["violations"].append((i, bad))
    return rep


def _near(v, thr, scale=LD(1)):
    """Within TOL (x scale) of the threshold without being equal to it."""
    d = np.abs(LD(v) - LD(thr))
    return bool(d != 0 and d <= TOL * scale)


def _wedge(m, k, l, p, hausd):
    """(accepted, undecidable) of the shadow wedge of local edge l of tria k."""
    c0 = np.asarray(m.xyz[m.tria[k, (l + 1) % 3]], LD)
    c1 = np.asarray(m.xyz[m.tria[k, (l + 2) % 3]], LD)
    a, pv = c1 - c0, p - c0
    a2, alpha = _dot(a, a), _dot(a, pv)
    r = pv - (alpha / a2) * a
    dist = np.sqrt(_dot(r, r))
    und = _near(alpha, 0, a2) or _near(alpha, a2, a2) or _near(dist, hausd)
    return bool(0 <= alpha <= a2 and dist <= hausd), und


def _cone(m, k, i, p, hausd, fan):
    """(accepted, undecidable, within hausd of the vertex) of the cone at local
    vertex i of tria k."""
    ip = int(m.tria[k, i])
    c0 = np.asarray(m.xyz[ip], LD)
    pv = p - c0
    dist = np.sqrt(_dot(pv, pv))
    near, und = bool(dist <= hausd), _near(dist, hausd)
    ok = near
    for t in fan.get(ip, ()):
        for jp in m.tria[t]:
            if jp == ip:
                continue
            a = np.asarray(m.xyz[jp], LD) - c0
            alpha = _dot(a, pv)
            ok &= bool(alpha <= 0)
            und |= _near(alpha, 0, _dot(a, a))
    return ok, und, near


def check_surface(m, x, elem, status, edge, vertex, ref=None):
    """The report of the surface answers (elem, status, edge, vertex) of the
    points x: counts per class (inside, border_edge, border_vertex, wedge, cone,
    cone_skip, exhaustive, not_found, undecidable), the violations on decidable
    points and `skipped`, the points of class cone_skip."""
    ref = surface_ref(m, x) if ref is None else ref
    assert ref["n"] == len(x) == len(elem) == len(status) == len(edge) == len(vertex)
    rep = _report(("inside", "border_edge", "border_vertex", "wedge", "cone", "cone_skip", "exhaustive", "not_found"))
    rep["skipped"] = []
    hausd, inT, nT = ref["hausd"], ref["inT"], ref["nT"]
    for i in range(len(x)):
        k, s, e, v = int(elem[i]), int(status[i]), int(edge[i]), int(vertex[i])
        und = bool(ref["und"][i])
        bad = cls = None
        if not (1 <= k <= m.nt and m.tria[k, 0] > 0):
            bad = f"tria {k} is not a valid tria"
        elif s == 0:
            cls = "not_found"
            if nT[i] > 0:
                bad = f"status 0 but {nT[i]} trias hold the point (first {np.argmax(inT[i])})"
            elif k != ref["nearest"][i]:
                bad = f"status 0 with tria {k}, the nearest centroid is tria {ref['nearest'][i]}'s"
        elif s == -1:
            cls = "exhaustive"
            if not inT[i, k]:
                bad = f"status -1 but tria {k} does not hold the point"
            elif e != -1 or v != -1:
                bad = f"status -1 with edge {e} / vertex {v}"
        elif s == 1 and (e not in (-1, 0, 1, 2) or v not in (-1, 0, 1, 2) or (e != -1 and v != -1)):
            bad = f"edge {e} / vertex {v}"
        elif s == 1:
            p = np.asarray(x[i], LD)
            lam, _ = tria_lambdas(m.xyz[m.tria[k]], p)
            o = np.argsort(lam, kind="stable")
            l0, l1 = lam[o[0]], lam[o[1]]
            if e == -1 and v == -1:
                cls = "inside"
                und |= _near(l0, EPS)
                if not inT[i, k]:
                    bad = f"tria {k} does not hold the point"
                elif not l0 >= EPS:
                    bad = f"min lambda {float(l0):.3g} < EPS but neither edge nor vertex"
            elif e != -1 and lam[e] > -EPS:
                cls = "border_edge"
                und |= _near(lam[e], -EPS) or _near(l0, EPS) or _near(l1, EPS)
                if not inT[i, k]:
                    bad = f"edge {e} with lambda {float(lam[e]):.3g} > -EPS but tria {k} does not hold the point"
                elif not (lam[e] == l0 and l0 < EPS and l1 >= EPS):
                    bad = f"edge {e} is not the border of tria {k}: lambda {[float(t) for t in lam]}"
            elif e != -1:
                cls = "wedge"
                ok, u = _wedge(m, k, e, p, hausd)
                und |= u or _near(lam[e], -EPS)
                if not ok:
                    bad = f"edge {e} of tria {k}: outside the shadow wedge"
            else:
                own = bool(inT[i, k] and l0 < EPS and l1 < EPS and v == o[2])
                if own:
                    cls = "border_vertex"
                    und |= _near(l0, EPS) or _near(l1, EPS)
                else:
                    ok, u, near = _cone(m, k, v, p, hausd, ref["fan"])
                    cls = "cone" if ok or not near else "cone_skip"
                    und |= u or (bool(inT[i, k]) and (_near(l0, EPS) or _near(l1, EPS)))
                    if not near:
                        bad = f"vertex {v} of tria {k}: neither the tria's own vertex nor inside the cone"
        else:
            bad = f"status {s}"
        if und:
            rep["undecidable"] += 1
            continue
        if cls:
            rep[cls] += 1
        if cls == "cone_skip":
            rep["skipped"].append(i)
        if bad:
            rep["violations"].append((i, bad))
    return rep
