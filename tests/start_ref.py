"""Where a walk starts, by definition (no tests here).

Plain numpy, written from the comments of setup_grids / size_tria_grid /
quant_xyz / hint_cell / walk_hint / tria_hint and include/pmx_transfer.h, for
what Transfer.debug_grid and Transfer.starts return.  Every quantity below is
a float64 subtract, multiply, add or divide in the kernels' order (the library
is built without contraction), or integer arithmetic: the expectation is
equality, nothing here has a tolerance.

A grid is (desc, cells): desc = {"dim", "qf", "lo", "inv"} and cells indexed
[z, y, x]; cell (x, y, z) is flat index x + dim[0] * (y + dim[1] * z).

Sizing (check_sizing): lo is the bounding-box minimum of the vertex rows
1..np bit for bit; inv[a] == dim[a] / (hi[a] - lo[a]); h is the cube root of
the box volume over max(1, ne / 6) (volume grid, cap 4096 per axis) or the
square root of the box area over max(1, nt / 8) (tria grid, cap 1024); an axis
whose ext / h exceeds the cap has dim == cap, every other axis has dim within
1 of ext / h (the library rounds up with a 1e-9 slack against libm's cbrt /
sqrt: the definition does not restate the rounding); the volume grid's
qf[a] == 21 - ceil(log2 dim[a]); the cells are dim[0] * dim[1] * dim[2].

Volume cells (check_volume_cells): the sample is tets 1, 1 + s, 1 + 2 s, ...
with a valid first vertex, s = hint_stride or 4 -- or, for a background
uploaded with PMX_HINT_SAMPLE_ORDER=2 and a step with the default stride, one
tet per vertex: the smallest valid tet among those whose smallest vertex it is.
cell_of(k) comes from the vertices' fixed-point coordinates: per axis
q = (x - lo) * inv * 2^qf truncated and clamped to [0, (dim << qf) - 1], the
four q summed, shifted right by qf + 2 and clamped to dim - 1.  A cell is
non-zero iff some sampled tet has cell_of == cell, and then holds one of them
(the kernel's plain store is racy: any of them is right).

Tria cells (check_tria_cells): each cell equals the largest valid tria whose
centroid ((a + b) + c) / 3 falls in it -- int(min(max((m - lo) * inv, 0),
dim - 1)) per axis -- and 0 elsewhere; the whole array is compared.

Starts (check_starts): a volume point starts at the tet of its clamped cell;
if that is 0, at the first non-zero cell of the shells r = 1..3 around it,
each scanned dz, dy, dx ascending over the cells with max(|dx|, |dy|, |dz|)
== r inside the grid; else at tet 1.  A surface point likewise on the tria
grid with r = 1..4.
"""
from __future__ import annotations

import numpy as np

VOL_CAP, TRIA_CAP = 4096, 1024
VOL_SHELLS, TRIA_SHELLS = 3, 4


# ---- sizing ------------------------------------------------------------------------

def bbox(m):
    x = m.xyz[1:m.np + 1]
    return x.min(axis=0), x.max(axis=0)


def check_sizing(m, desc, ncells, which):
    """The violations (strings) of a downloaded descriptor against the sizing
    rules; which 0 the volume grid, 1 the tria grid."""
    bad = []
    lo, hi = bbox(m)
    dim = np.asarray(desc["dim"], np.int64)
    if not np.array_equal(np.asarray(desc["lo"], np.float64).view(np.int64), lo.view(np.int64)):
        bad.append(f"lo {desc['lo']} is not the bounding-box minimum {lo}")
    ext = np.maximum(hi - lo, 1e-300)
    inv = dim.astype(np.float64) / ext
    if not np.array_equal(np.asarray(desc["inv"], np.float64).view(np.int64), inv.view(np.int64)):
        bad.append(f"inv {desc['inv']} != dim / ext {inv}")
    if which == 0:
        h = np.cbrt(ext[0] * ext[1] * ext[2] / max(1.0, m.ne / 6.0))
        cap = VOL_CAP
    else:
        h = np.sqrt(2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) / max(1.0, m.nt / 8.0))
        cap = TRIA_CAP
    for a in range(3):
        want = ext[a] / h
        if want > cap:
            if dim[a] != cap:
                bad.append(f"axis {a}: ext / h = {want} exceeds the cap, dim {dim[a]} != {cap}")
        elif not (1 <= dim[a] <= cap and abs(dim[a] - want) <= 1.0):
            bad.append(f"axis {a}: dim {dim[a]} is not within 1 of ext / h = {want}")
        if which == 0:
            bits = int(dim[a] - 1).bit_length()             # ceil(log2 dim)
            if desc["qf"][a] != 21 - bits:
                bad.append(f"axis {a}: qf {desc['qf'][a]} != 21 - ceil(log2 {dim[a]})")
    if int(dim.prod()) != int(ncells):
        bad.append(f"{ncells} cells for dims {dim}")
    return bad


def nominal_desc(m, which):
    """The descriptor the sizing rules give on this host (libm's cbrt / sqrt,
    rounded up with the library's 1e-9 slack): for the conditions the tests
    check on the CPU before a device run.  A device grid is held to
    check_sizing, not to this."""
    lo, hi = bbox(m)
    ext = np.maximum(hi - lo, 1e-300)
    if which == 0:
        h, cap = np.cbrt(ext[0] * ext[1] * ext[2] / max(1.0, m.ne / 6.0)), VOL_CAP
    else:
        h = np.sqrt(2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) / max(1.0, m.nt / 8.0))
        cap = TRIA_CAP
    dim = np.clip(np.ceil(ext / h * (1.0 - 1e-9)).astype(np.int64), 1, cap)
    qf = np.array([21 - int(d - 1).bit_length() for d in dim], np.int64) if which == 0 else np.zeros(3, np.int64)
    return {"dim": dim, "qf": qf, "lo": lo.copy(), "inv": dim.astype(np.float64) / ext}


# ---- volume cells --------------------------------------------------------------------

def sample(m, stride=0, order=0):
    """The 1-based tets the step's hint build reads (sorted)."""
    valid = m.tet[:, 0] > 0
    valid[0] = False
    if order == 2 and stride in (0, 4):
        ks = np.nonzero(valid)[0]
        vmin = m.tet[ks].min(axis=1)
        owner = np.full(m.np + 1, np.iinfo(np.int64).max)
        np.minimum.at(owner, vmin, ks)
        return np.sort(owner[owner <= m.ne])
    s = stride if stride > 0 else 4
    ks = np.arange(1, m.ne + 1, s)
    return ks[valid[ks]]


def quant(m, desc):
    """(np+1, 3) int64: the vertices' fixed-point grid coordinates."""
    dim, qf = np.asarray(desc["dim"], np.int64), np.asarray(desc["qf"], np.int64)
    t = (m.xyz - desc["lo"][None]) * desc["inv"][None] * (1 << qf).astype(np.float64)[None]
    top = ((dim << qf) - 1).astype(np.float64)
    return np.minimum(np.where(t > 0.0, t, 0.0), top[None]).astype(np.int64)


def cell_of(m, desc, ks):
    """Flat cell of the tets ks from their vertices' fixed-point coordinates."""
    dim, qf = np.asarray(desc["dim"], np.int64), np.asarray(desc["qf"], np.int64)
    s4 = quant(m, desc)[m.tet[ks]].sum(axis=1)
    c = np.minimum(s4 >> (qf + 2)[None], dim[None] - 1)
    return c[:, 0] + dim[0] * (c[:, 1] + dim[1] * c[:, 2])


def check_volume_cells(m, desc, cells, stride=0, order=0):
    """The violations of a downloaded volume grid."""
    g = np.asarray(cells).ravel().astype(np.int64)
    ks = sample(m, stride, order)
    ck = cell_of(m, desc, ks)
    want = np.zeros(len(g), bool)
    want[ck] = True
    bad = []
    stale = np.nonzero((g != 0) & ~want)[0]
    empty = np.nonzero((g == 0) & want)[0]
    if len(stale):
        bad.append(f"{len(stale)} cells without a sampled tet are non-zero, first {stale[:5]} -> {g[stale[:5]]}")
    if len(empty):
        bad.append(f"{len(empty)} cells with a sampled tet are empty, first {empty[:5]}")
    home = np.full(m.ne + 1, -1, np.int64)               # sampled tet -> its cell
    home[ks] = ck
    nz = np.nonzero(g != 0)[0]
    inr = (g[nz] >= 1) & (g[nz] <= m.ne)
    if not inr.all():
        bad.append(f"{(~inr).sum()} cells hold no tet index 1..ne, first {g[nz[~inr][:5]]}")
    nz = nz[inr]
    wrong = nz[home[g[nz]] != nz]
    if len(wrong):
        bad.append(f"{len(wrong)} cells hold a tet that is not a sampled tet of that cell, first "
                   f"{wrong[:5]} -> {g[wrong[:5]]} (cells {home[g[wrong[:5]]]})")
    return bad


def some_volume_cells(m, desc, stride=0, order=0, pick=max):
    """A grid that obeys the definition: per cell the smallest / largest sampled tet."""
    dim = np.asarray(desc["dim"], np.int64)
    g = np.zeros(int(dim.prod()), np.int64)
    ks = sample(m, stride, order)
    ck = cell_of(m, desc, ks)
    if pick is max:
        np.maximum.at(g, ck, ks)
    else:
        g[ck[::-1]] = ks[::-1]
    return g.astype(np.int32).reshape(dim[2], dim[1], dim[0])


# ---- tria cells -------------------------------------------------------------------------

def _cell_coords(p, desc):
    """int(min(max((p - lo) * inv, 0), dim - 1)) per axis, (n, 3)."""
    dim = np.asarray(desc["dim"], np.int64)
    t = (np.asarray(p, np.float64) - desc["lo"][None]) * desc["inv"][None]
    return np.minimum(np.maximum(t, 0.0), (dim - 1).astype(np.float64)[None]).astype(np.int64)


def tria_cells(m, desc):
    """The tria grid by definition, [z, y, x]."""
    dim = np.asarray(desc["dim"], np.int64)
    g = np.zeros(int(dim.prod()), np.int64)
    ks = np.nonzero(m.tria[:, 0] > 0)[0]
    ks = ks[ks >= 1]
    P = m.xyz[m.tria[ks]]
    cen = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0
    c = _cell_coords(cen, desc)
    np.maximum.at(g, c[:, 0] + dim[0] * (c[:, 1] + dim[1] * c[:, 2]), ks)
    return g.astype(np.int32).reshape(dim[2], dim[1], dim[0])


def check_tria_cells(m, desc, cells):
    want = tria_cells(m, desc)
    got = np.asarray(cells).reshape(want.shape)
    diff = np.argwhere(got != want)
    if len(diff):
        z, y, x = diff[0]
        return [f"{len(diff)} tria cells differ, first (x, y, z) = ({x}, {y}, {z}): {got[z, y, x]} != {want[z, y, x]}"]
    return []


# ---- starts ----------------------------------------------------------------------------------

def _shell(r, order="zyx"):
    """The offsets (dx, dy, dz) of shell r in scan order; order names the
    loops from the outermost to the innermost."""
    rng = range(-r, r + 1)
    out = []
    for a in rng:
        for b in rng:
            for c in rng:
                d = dict(zip(order, (a, b, c)))
                if max(abs(d["x"]), abs(d["y"]), abs(d["z"])) == r:
                    out.append((d["x"], d["y"], d["z"]))
    return out


def hint_starts(desc, cells, p, shells, order="zyx"):
    """The start element of every point p (n, 3) on a grid: (start (n,),
    radius (n,)) with radius 0 the point's own cell, 1..shells the shell that
    answered, -1 no non-zero cell within reach (start 1)."""
    dim = [int(d) for d in desc["dim"]]
    g = np.asarray(cells).reshape(dim[2], dim[1], dim[0])
    c = _cell_coords(p, desc)
    start = np.ones(len(c), np.int64)
    radius = np.full(len(c), -1, np.int64)
    offs = {r: _shell(r, order) for r in range(1, shells + 1)}
    for i, (cx, cy, cz) in enumerate(c):
        k = g[cz, cy, cx]
        if k:
            start[i], radius[i] = k, 0
            continue
        for r in range(1, shells + 1):
            for dx, dy, dz in offs[r]:
                x, y, z = cx + dx, cy + dy, cz + dz
                if x < 0 or y < 0 or z < 0 or x >= dim[0] or y >= dim[1] or z >= dim[2]:
                    continue
                if g[z, y, x]:
                    start[i], radius[i] = g[z, y, x], r
                    break
            if radius[i] > 0:
                break
    return start, radius


def expected_starts(x, tags, vgrid, tgrid, bdy_bit=16, **kw):
    """The starts of a hint-grid step from its downloaded grids: volume
    points (tag without bdy_bit) on vgrid = (desc, cells) with 3 shells,
    surface points on tgrid (None: no surface points) with 4.  Returns
    (start (n,), radius (n,))."""
    x = np.asarray(x, np.float64)
    isb = (np.asarray(tags) & bdy_bit) != 0
    start = np.zeros(len(x), np.int64)
    radius = np.zeros(len(x), np.int64)
    start[~isb], radius[~isb] = hint_starts(vgrid[0], vgrid[1], x[~isb], VOL_SHELLS, **kw)
    if isb.any():
        start[isb], radius[isb] = hint_starts(tgrid[0], tgrid[1], x[isb], TRIA_SHELLS, **kw)
    return start, radius


def check_starts(x, tags, starts, vgrid, tgrid):
    want, _ = expected_starts(x, tags, vgrid, tgrid)
    diff = np.nonzero(np.asarray(starts, np.int64) != want)[0]
    if len(diff):
        return [f"{len(diff)} starts are not the grid's, first points {diff[:5]}: "
                f"{np.asarray(starts)[diff[:5]]} != {want[diff[:5]]}"]
    return []
