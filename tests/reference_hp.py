"""An independent high-precision reference of the tensor formulas (no tests here).

Plain numpy, evaluated in ``np.longdouble`` (and, for the noise floor, again in
float64: every function takes ``dtype``).  Written from the definitions, not
from the oracle: full 3x3 matrices, einsum, cross-product (adjugate) inverses.
The only knowledge of the 6-component storage is :func:`full`, which maps
(m11, m12, m13, m22, m23, m33) to the symmetric matrix; results that are
matrices stay matrices, and the callers compare them with ``full(row)``.

Definitions

* interpolation of a metric: (sum_i lambda_i M_i^-1)^-1, of a scalar / vector:
  sum_i lambda_i u_i, lambda the barycentrics of the point in its element;
* Mmg's documented MMG5_invmat rule: a matrix whose largest off-diagonal
  magnitude is below 1e-6 (absolute) is inverted as its diagonal; one with
  |det| < 1e-200 does not invert and the row is not written;
* quality: vol / (sum |e|^2)^(3/2), in a metric sqrt(det Mbar) vol /
  (sum e^T Mbar e)^(3/2) with Mbar the mean vertex metric and vol the triple
  product (6 x the volume); 0 when vol <= 0;
* edge length: |e| / h1 if |h2/h1 - 1| < 1e-6, else |e| log1p(h2/h1 - 1) /
  (h2 - h1); in a metric (sqrt d1 + sqrt d2 + 4 sqrt((d1 + d2)/2)) / 6 with
  d_i = e^T M_i e clamped at 0.
"""
from __future__ import annotations

import numpy as np
import pytest

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:            # no extended precision on this platform
    pytest.skip("np.longdouble is not wider than float64 here", allow_module_level=True)
assert np.finfo(LD).eps < 1e-18

ALPHAD = 20.7846097
INV_DIAG = 1e-6          # MMG5_invmat: below this, the off-diagonals are dropped
INV_DET = 1e-200         # ... and below this |det| the inversion fails
LEN_BOUNDS = (0.0, 0.3, 0.6, 0.7071, 0.9, 1.3, 1.4142, 2.0, 5.0)
QUAL_BOUNDS = (0.2, 0.4, 0.6, 0.8)
TAG_GEO, TAG_REQ, TAG_NOM, TAG_CRN = 2, 4, 8, 32
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def full(m6, dtype=LD):
    """(..., 6) rows (m11, m12, m13, m22, m23, m33) -> (..., 3, 3) matrices."""
    m = np.asarray(m6, dtype)
    a, b, c, d, e, f = (m[..., k] for k in range(6))
    return np.stack([np.stack([a, b, c], -1), np.stack([b, d, e], -1), np.stack([c, e, f], -1)], -2)


def _det_adj(A):
    """Determinant and adjugate of (..., 3, 3) matrices by cross products."""
    r0, r1, r2 = A[..., 0, :], A[..., 1, :], A[..., 2, :]
    adj = np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], -1)   # columns
    det = np.einsum("...i,...i->...", r0, np.cross(r1, r2))
    return det, adj


def _solve3(A, r):
    """A x = r for (..., 3, 3) / (..., 3), adjugate inverse + one refinement."""
    det, adj = _det_adj(A)
    inv = adj / det[..., None, None]
    x = np.einsum("...ij,...j->...i", inv, r)
    x = x + np.einsum("...ij,...j->...i", inv, r - np.einsum("...ij,...j->...i", A, x))
    return x


def bary_tet(P, x, dtype=LD):
    """Barycentrics (N, 4) of points x (N, 3) in tets P (N, 4, 3)."""
    P, x = np.asarray(P, dtype), np.asarray(x, dtype)
    A = np.swapaxes(P[:, 1:] - P[:, :1], -1, -2)          # columns p_i - p_0
    mu = _solve3(A, x - P[:, 0])
    return np.concatenate([1 - mu.sum(-1, keepdims=True), mu], -1)


def bary_tria(P, x, dtype=LD):
    """Barycentrics (N, 3) of the orthogonal projections of x (N, 3) on the
    planes of trias P (N, 3, 3): least squares in the plane."""
    P, x = np.asarray(P, dtype), np.asarray(x, dtype)
    E = P[:, 1:] - P[:, :1]                               # (N, 2, 3)
    G = np.einsum("nik,njk->nij", E, E)
    det = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]

    def solve(r):
        b = np.einsum("nik,nk->ni", E, r)
        return np.stack([G[:, 1, 1] * b[:, 0] - G[:, 0, 1] * b[:, 1],
                         G[:, 0, 0] * b[:, 1] - G[:, 1, 0] * b[:, 0]], -1) / det[:, None]
    r = x - P[:, 0]
    mu = solve(r)
    mu = mu + solve(r - np.einsum("ni,nik->nk", mu, E))
    return np.concatenate([1 - mu.sum(-1, keepdims=True), mu], -1)


def bary_edge(P, x, dtype=LD):
    """Barycentrics (N, 2) of the projections of x on the lines through P (N, 2, 3)."""
    P, x = np.asarray(P, dtype), np.asarray(x, dtype)
    e = P[:, 1] - P[:, 0]
    t = np.einsum("nk,nk->n", x - P[:, 0], e) / np.einsum("nk,nk->n", e, e)
    return np.stack([1 - t, t], -1)


def invmat(A, diag_rule=True):
    """MMG5_invmat's rule on (..., 3, 3) matrices -> (inverse, ok).
    diag_rule=False: the plain inverse (to show that the rule matters)."""
    off = np.max(np.abs(np.stack([A[..., 0, 1], A[..., 0, 2], A[..., 1, 2]], -1)), -1)
    diag = (off < INV_DIAG) & diag_rule
    D = np.zeros_like(A)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(3):
            D[..., k, k] = 1 / A[..., k, k]
        det, adj = _det_adj(A)
        ok = diag | ~(np.abs(det) < INV_DET)
        inv = adj / det[..., None, None]
    return np.where(diag[..., None, None], D, inv), ok


def interp_rows(lam, rows, dtype=LD, diag_rule=True):
    """lam (N, k) weights, rows (N, k, size) the element's vertex rows.
    size 1 / 3: (N, size) sums; size 6: ((N, 3, 3) matrices, written (N,) bool)."""
    lam, rows = np.asarray(lam, dtype), np.asarray(rows, dtype)
    if rows.shape[-1] != 6:
        return np.einsum("nk,nks->ns", lam, rows)
    inv, ok = invmat(full(rows, dtype), diag_rule)
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.einsum("nk,nkij->nij", lam, inv)
    out, ok2 = invmat(S, diag_rule)
    return out, ok.all(-1) & ok2


def interp_at(m, x, tags, elem, status, sol, dtype=LD, diag_rule=True, edge=None, vert=None, metric=False):
    """The interpolation of `sol` ((np+1, size), Mmg layout) at the points x
    (n, 3) in the elements a transfer located them in: elem the 1-based tet
    (tags without MG_BDY) or boundary tria, status 0 = no element contains the
    point and the closest element's vertex nearest to it gives the value
    (barycentrics 1, 0, 0, 0).  edge / vert (-1: none): a surface point that
    ended on local edge l or vertex i of its tria.  The metric (metric=True)
    is then interpolated along the edge / copied from the vertex; an edge
    reached from outside the tria (its barycentric below -1e-6) weighs every
    field by the projection on the edge.  Returns (values, written): (n, size)
    rows or (n, 3, 3) matrices, and which rows the definition writes."""
    x = np.asarray(x, np.float64)
    n, size = len(x), sol.shape[1]
    out = np.zeros((n, 3, 3) if size == 6 else (n, size), dtype)
    written = np.ones(n, bool)
    bdy = (np.asarray(tags).astype(np.int64) & 16) != 0
    for sel, conn, bary in ((~bdy, m.tet, bary_tet), (bdy, m.tria, bary_tria)):
        idx = np.nonzero(sel)[0]
        if not len(idx):
            continue
        v = conn[elem[idx]]
        P = m.xyz[v]
        lam = bary(P, x[idx], dtype)
        far = np.nonzero(status[idx] == 0)[0]
        if len(far):
            d = ((P[far] - x[idx[far], None, :]) ** 2).sum(-1)
            lam[far] = np.eye(v.shape[1], dtype=dtype)[np.argmin(d, axis=1)]
        if conn is m.tria and edge is not None:
            for j in np.nonzero(edge[idx] != -1)[0]:
                l = int(edge[idx[j]])
                i0, i1 = (l + 1) % 3, (l + 2) % 3
                if lam[j, l] <= -1e-6:                    # reached through the neighbour's wedge
                    lam[j, [i0, i1]] = bary_edge(P[j:j + 1, [i0, i1]], x[idx[j:j + 1]], dtype)[0]
                    lam[j, l] = 0
                elif metric:
                    lam[j, l] = 0
        r = interp_rows(lam, sol[v], dtype, diag_rule)
        if size == 6:
            out[idx], written[idx] = r
        else:
            out[idx] = r
        if conn is m.tria and vert is not None and metric:
            for j in np.nonzero(vert[idx] != -1)[0]:
                row = sol[v[j, int(vert[idx[j]])]]
                out[idx[j]] = full(row, dtype) if size == 6 else np.asarray(row, dtype)
                written[idx[j]] = True
    return out, written


def _vol_edges(P):
    a, b, c, d = (P[:, k] for k in range(4))
    vol = np.einsum("nk,nk->n", b - a, np.cross(c - a, d - a))
    E = np.stack([P[:, j] - P[:, i] for i, j in PAIRS], 1)            # (N, 6, 3)
    return vol, E


def qual_iso(P, dtype=LD):
    vol, E = _vol_edges(np.asarray(P, dtype))
    rap = np.einsum("nek,nek->n", E, E)
    return np.where(vol > 0, vol / (rap * np.sqrt(rap)), 0)


def _qual_mean(P, Mbar, none):
    vol, E = _vol_edges(P)
    det, _ = _det_adj(Mbar)
    rap = np.einsum("nei,nij,nej->n", E, Mbar, E)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.sqrt(det) * vol / (rap * np.sqrt(rap))
    return np.where((vol > 0) & ~none, q, 0)


def qual_ani(P, M, dtype=LD):
    """P (N, 4, 3), M (N, 4, 6): the mean of the four vertex metrics."""
    Mbar = full(M, dtype).sum(1) / 4
    return _qual_mean(np.asarray(P, dtype), Mbar, np.zeros(len(Mbar), bool))


def is_ridge(tags):
    """Non-singular ridge points: MG_GEO without MG_CRN, MG_REQ, MG_NOM."""
    t = np.asarray(tags).astype(np.int64)
    return ((t & TAG_GEO) != 0) & ((t & (TAG_CRN | TAG_REQ | TAG_NOM)) == 0)


def qual_ani_ridge(P, M, ridge, dtype=LD):
    """ridge (N, 4) bool: the mean over the vertices that are not ridge points."""
    keep = ~np.asarray(ridge, bool)
    n = keep.sum(1)
    Mf = full(M, dtype)
    Mbar = np.einsum("nk,nkij->nij", keep.astype(dtype), Mf) / np.maximum(n, 1).astype(dtype)[:, None, None]
    none = n == 0
    Mbar[none] = np.eye(3, dtype=dtype)
    return _qual_mean(np.asarray(P, dtype), Mbar, none)


def qual_stats(q, tets=None, tags=None):
    """Statistics of the qualities q (N,) of the valid tets (row k = tet k+1);
    tets (N, 4) + point tags: nrid, the tets whose 4 vertices are ridge points."""
    rap = ALPHAD * np.asarray(q)
    ir = np.minimum((5 * rap).astype(np.int64), 4)
    k = int(np.argmin(rap))
    d = dict(ne=len(rap), min=rap[k], iel=k + 1, max=rap.max(), avg=rap.sum(), good=int((rap > 0.12).sum()),
             med=int((rap > 0.5).sum()), his=[int((ir == b).sum()) for b in range(5)], nrid=0)
    if tags is not None:
        d["nrid"] = int(is_ridge(tags)[tets].all(1).sum())
    return d


def unique_edges(tets, tags=None):
    """Unique edges (min, max) of the tets (N, 4), without the tets whose four
    vertices are ridge points."""
    t = np.asarray(tets, np.int64)
    if tags is not None:
        t = t[~is_ridge(tags)[t].all(1)]
    e = np.concatenate([np.sort(t[:, [i, j]], 1) for i, j in PAIRS])
    return np.unique(e, axis=0)


def len_iso(xyz, h, edges, dtype=LD):
    x, h = np.asarray(xyz, dtype), np.asarray(h, dtype).reshape(-1)
    e = x[edges[:, 1]] - x[edges[:, 0]]
    l = np.sqrt(np.einsum("nk,nk->n", e, e))
    h1, h2 = h[edges[:, 0]], h[edges[:, 1]]
    r = h2 / h1 - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.abs(r) < 1e-6, l / h1, l * np.log1p(r) / (h2 - h1))


def len_ani33(xyz, met, edges, dtype=LD):
    x, M = np.asarray(xyz, dtype), full(met, dtype)
    e = x[edges[:, 1]] - x[edges[:, 0]]
    d1 = np.maximum(np.einsum("ni,nij,nj->n", e, M[edges[:, 0]], e), 0)
    d2 = np.maximum(np.einsum("ni,nij,nj->n", e, M[edges[:, 1]], e), 0)
    return (np.sqrt(d1) + np.sqrt(d2) + 4 * np.sqrt((d1 + d2) / 2)) / 6


def len_stats(lengths, edges):
    l = np.asarray(lengths)
    nz = l != 0
    lc, ec = l[nz], np.asarray(edges)[nz]
    b = LEN_BOUNDS
    hl = [int(((lc >= b[i]) & (lc < b[i + 1])).sum()) for i in range(8)] + [int((lc >= b[8]).sum())]
    i0, i1 = int(np.argmin(lc)), int(np.argmax(lc))
    return dict(ned=len(lc), nullEdge=int((~nz).sum()), avlen=lc.sum(), lmin=lc[i0], lmax=lc[i1],
                emin={int(ec[i0, 0]), int(ec[i0, 1])}, emax={int(ec[i1, 0]), int(ec[i1, 1])}, hl=hl)


def clear_of(values, bounds, rel=1e-9):
    """True when no value lies within rel (relative) of one of the bounds."""
    v = np.asarray(values, LD)[:, None]
    b = np.asarray([x for x in bounds if x != 0], LD)[None, :]
    return bool(np.all(np.abs(v - b) > rel * b))


def rel_rows(A, B):
    """Per row: max |A - B| over the row, relative to the largest |B| entry."""
    A, B = np.asarray(A, LD), np.asarray(B, LD)
    n = len(A)
    d = np.abs(A - B).reshape(n, -1).max(1)
    return d / np.abs(B).reshape(n, -1).max(1)


# ---- comparisons shared by the CPU and the GPU tests ---------------------------
# The tolerance of every quantity is 8 x its noise floor: the largest deviation
# between this reference in float64 and in long double on the same inputs.

SENT = -7.0          # the value of a row nobody wrote


def interp_errors(m, x, t, elem, status, sol, got, **kw):
    """(floor, error of `got`, written) of the interpolation of sol, per point
    and relative to the row's largest entry; the rows the definition does not
    write must be the rows `got` left at SENT (they are in neither figure)."""
    ref, w = interp_at(m, x, t, elem, status, sol, LD, **kw)
    r64, w64 = interp_at(m, x, t, elem, status, sol, np.float64, **kw)
    assert np.array_equal(w, w64)
    untouched = (got == SENT).all(axis=1)
    assert np.array_equal(untouched, ~w), "rows left unwritten differ from the definition's"
    g = full(got) if sol.shape[1] == 6 else got
    return rel_rows(r64[w], ref[w]), rel_rows(g[w], ref[w]), w


def quality_errors(P, M4, got, ridge=None):
    """(reference, floor, error of `got`) of the qualities of tets P (N, 4, 3)
    in the vertex metrics M4 (N, 4, 6) or None; ridge (N, 4): the mean metric
    without those vertices.  Relative, over the tets of positive quality; the
    others must be exactly 0 in `got`."""
    if M4 is None:
        ref, r64 = qual_iso(P), qual_iso(P, np.float64)
    elif ridge is None:
        ref, r64 = qual_ani(P, M4), qual_ani(P, M4, np.float64)
    else:
        ref, r64 = qual_ani_ridge(P, M4, ridge), qual_ani_ridge(P, M4, ridge, np.float64)
    pos = ref > 0
    got = np.asarray(got)
    assert np.all(got[~pos] == 0.0) and np.all(r64[~pos] == 0)
    return ref, np.abs(r64[pos] - ref[pos]) / ref[pos], np.abs(got[pos] - ref[pos]) / ref[pos]


def check_qual_stats(h, ref, tets, tags, tol):
    """Statistics h (oracle or device) against the reference qualities."""
    assert clear_of(ALPHAD * ref, QUAL_BOUNDS + (0.12, 0.5))
    s = qual_stats(ref, tets, tags)
    for f in ("ne", "iel", "good", "med", "his", "nrid"):
        assert h[f] == s[f], (f, h[f], s[f])
    for f in ("min", "max"):
        assert abs(h[f] - s[f]) <= tol * abs(s[f]), f
    assert abs(h["avg"] - s["avg"]) <= 1e-12 * abs(s["avg"])


def length_reference(m, met, tags=None):
    """(edges, reference lengths, noise floor) of a size-1 or size-6 metric."""
    ed = unique_edges(m.tet[1:][m.tet[1:, 0] > 0], tags)
    f = len_ani33 if met.shape[1] == 6 else len_iso
    ref, r64 = f(m.xyz, met, ed), f(m.xyz, met, ed, np.float64)
    return ed, ref, float((np.abs(r64 - ref) / ref).max())


def check_len_stats(L, ed, ref, tol):
    """Statistics L (oracle or device) against the reference lengths."""
    assert clear_of(ref, LEN_BOUNDS)
    s = len_stats(ref, ed)
    assert (L["ned"], L["nullEdge"], L["hl"]) == (s["ned"], s["nullEdge"], s["hl"]), (L, s)
    assert abs(L["lmin"] - s["lmin"]) <= tol * s["lmin"] and abs(L["lmax"] - s["lmax"]) <= tol * s["lmax"]
    assert {L["amin"], L["bmin"]} == s["emin"] and {L["amax"], L["bmax"]} == s["emax"]
    assert abs(L["avlen"] - s["avlen"]) <= 1e-12 * abs(s["avlen"])
    return s
