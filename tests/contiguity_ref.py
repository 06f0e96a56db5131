"""The CPU twin of pmx_contiguity / pmx_fix_contiguity
(tests/c/contiguity_ref.c) through ctypes, and the partitions the contiguity
tests share (test infrastructure).  The twin is UNPINNED: Mmg is absent, so the
reference file it restates cannot be built here."""
import ctypes as C
import os
import subprocess

import numpy as np

from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "contiguity_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libcontiguity_ref.so")

_lib = None


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("ncomp", "nmerged", "nmerged_tets", "ncannot", "counter")]


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
        l.cgr_components.restype = i64
        l.cgr_components.argtypes = [i64, vp, vp, C.c_int, vp, vp]
        l.cgr_sweep_group.restype = C.c_int
        l.cgr_sweep_group.argtypes = [i64, vp]
        l.cgr_sweep_parts.restype = C.c_int
        l.cgr_sweep_parts.argtypes = [i64, vp, vp, vp, C.c_int, vp]
        l.cgr_fix.restype = None
        l.cgr_fix.argtypes = [i64, vp, vp, C.c_int, vp, C.POINTER(Stats)]
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _mark1(part, ne):
    """part (ne,) -> the 1-based mark array (slot 0 unused)."""
    mk = np.zeros(ne + 1, np.int32)
    mk[1:] = part
    return mk


def components(m, part=None, nparts=1):
    """(ncomp, counts (nparts,), label (ne,)) by breadth-first search."""
    ne = m.ne
    adja = np.ascontiguousarray(m.adja, np.int32)
    mk = None if part is None else _mark1(part, ne)
    counts = np.zeros(nparts, np.int32)
    label = np.zeros(ne + 1, np.int32)
    n = lib().cgr_components(ne, _p(adja), _p(mk), nparts, _p(counts), _p(label))
    return int(n), counts, label[1:].copy()


def sweep_group(m):
    return int(lib().cgr_sweep_group(m.ne, _p(np.ascontiguousarray(m.adja, np.int32))))


def sweep_parts(m, part, nparts):
    """(the reference's return value: the last part's count, counts)."""
    xadj, adjncy = numpy_graph(m)
    p = np.ascontiguousarray(part, np.int32)
    counts = np.zeros(nparts, np.int32)
    r = lib().cgr_sweep_parts(m.ne, _p(xadj), _p(adjncy), _p(p), nparts, _p(counts))
    return int(r), counts


def fix(m, part, colors_or_n):
    """FIX on a copy of part: (part, stats dict); ncomp counted before the fix."""
    ne = m.ne
    adja = np.ascontiguousarray(m.adja, np.int32)
    col = (np.arange(colors_or_n, dtype=np.int32) if np.ndim(colors_or_n) == 0
           else np.ascontiguousarray(colors_or_n, np.int32))
    mk = _mark1(part, ne)
    st = Stats()
    st.ncomp = components(m, part, 1)[0]
    lib().cgr_fix(ne, _p(adja), _p(mk), len(col), _p(col), C.byref(st))
    return mk[1:].copy(), {f: getattr(st, f) for f, _ in st._fields_}


def numpy_graph(m):
    """xadj / adjncy (0-based nodes) straight from m.adja."""
    ne = m.ne
    a = m.adja[1:4 * ne + 1].reshape(ne, 4) // 4
    on = a != 0
    xadj = np.zeros(ne + 1, np.int32)
    xadj[1:] = np.cumsum(on.sum(1))
    return xadj, np.ascontiguousarray((a[on] - 1).astype(np.int32))


def numpy_labels(m, part=None):
    """Independent of the twin: iterate label[k] = min over same-colour
    neighbours until nothing changes; (ncomp, label (ne,))."""
    ne = m.ne
    nb = m.adja[1:4 * ne + 1].reshape(ne, 4) // 4          # 1-based, 0 none
    p = np.zeros(ne + 1, np.int64) if part is None else np.concatenate([[-(1 << 40)], np.asarray(part, np.int64)])
    ok = (nb != 0) & (p[nb] == p[1:, None])
    lab = np.arange(ne + 1, dtype=np.int64)
    while True:
        cand = np.where(ok, lab[nb], ne + 1)
        new = lab.copy()
        new[1:] = np.minimum(lab[1:], cand.min(1))
        new = new[new]                                      # pointer jumping
        if np.array_equal(new, lab):
            break
        lab = new
    return len(np.unique(lab[1:])), lab[1:].astype(np.int32)


# ---- meshes and partitions ----------------------------------------------------------

def cells(m, n):
    """Integer cell coordinates (ne, 3) of the tets of kuhn_cube(n)."""
    return np.minimum((m.centroids() * n).astype(np.int64), n - 1)


def slabs(m, nparts):
    """z-slabs of equal thickness."""
    z = m.centroids()[:, 2]
    return np.minimum((z * nparts).astype(np.int32), nparts - 1)


def boustrophedon(m, n):
    """Colour 1 on a one-cell-thick path through the cube that turns back and
    forth in x, then y, leaving one-cell gaps, colour 0 elsewhere: the path's
    graph diameter is of the order of its cell count."""
    c = cells(m, n)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    on_row = (y % 2 == 0) & (z % 2 == 0)
    # connectors between rows at alternating x ends, between layers at alternating y ends
    row = y // 2
    xend = np.where(row % 2 == 0, n - 1, 0)
    conn_y = (y % 2 == 1) & (z % 2 == 0) & (x == xend) & (y < n - 1)
    lay = z // 2
    nrow = (n + 1) // 2
    last_row_y = np.where(lay % 2 == 0, 2 * (nrow - 1), 0)
    # the free end of the row the path leaves a layer by: the last row's in
    # even layers, row 0's (x = 0) in odd ones
    xl = np.where(lay % 2 == 0, n - 1 if (nrow - 1) % 2 == 0 else 0, 0)
    conn_z = (z % 2 == 1) & (y == last_row_y) & (x == xl) & (z < n - 1)
    return (on_row | conn_y | conn_z).astype(np.int32)


def two_cubes(n1, n2):
    """kuhn_cube(n1) and kuhn_cube(n2), the second shifted by 2 in x, as one
    mesh with two face-connected components; returns (mesh, ne of the first)."""
    a, b = M.kuhn_cube(n1), M.kuhn_cube(n2, seed=77)
    xyz = np.concatenate([a.xyz, b.xyz[1:] + [2.0, 0.0, 0.0]])
    tet = np.concatenate([a.tet, b.tet[1:] + a.np])
    return M.from_tets(xyz, tet.astype(np.int32)), a.ne


def nearest(m, x, y, z):
    """The 0-based tet whose centroid is nearest to (x, y, z)."""
    return int(np.argmin(((m.centroids() - [x, y, z]) ** 2).sum(1)))


def plant(m, part, seeds, colour, size):
    """Recolour a face-connected blob of `size` tets grown breadth-first from
    each 0-based tet of seeds; returns the tets changed."""
    ne = m.ne
    nb = m.adja[1:4 * ne + 1].reshape(ne, 4) // 4
    changed = []
    for s in seeds:
        blob, q = [int(s)], [int(s)]
        seen = {int(s)}
        while q and len(blob) < size:
            k = q.pop(0)
            for k1 in nb[k]:
                if k1 and (k1 - 1) not in seen and len(blob) < size:
                    seen.add(int(k1 - 1))
                    blob.append(int(k1 - 1))
                    q.append(int(k1 - 1))
        part[blob] = colour
        changed += blob
    return changed


# ---- the planted cases (shared by the CPU and the GPU tests) ---------------------------

_cases = {}


def _planted12():
    """3 z-slabs of the n = 12 cube with fragments: colour 0 inside colour 2
    (target not yet processed) and colour 2 inside colour 0 (target already
    processed) as single tets, pairs and blobs; a colour-0 blob across the
    boundary of colours 1 and 2 (list order decides the target); a blob in a
    corner of the domain; a 3 x 3 x 3-cell block of colour 2 in the corner
    where the numbering starts, so that its list begins cells away from its
    only foreign neighbours (a long replay); colour 3 as two pieces of equal
    size."""
    m = M.kuhn_cube(12)
    part = slabs(m, 3)
    pick = lambda x, y, z: nearest(m, x, y, z)
    plant(m, part, [pick(0.2, 0.2, 0.85), pick(0.7, 0.3, 0.8)], 0, 1)
    plant(m, part, [pick(0.5, 0.5, 0.9), pick(0.3, 0.8, 0.75)], 0, 2)
    plant(m, part, [pick(0.8, 0.8, 0.85)], 0, 9)
    plant(m, part, [pick(0.2, 0.7, 0.15), pick(0.6, 0.6, 0.2)], 2, 1)
    plant(m, part, [pick(0.4, 0.2, 0.1)], 2, 2)
    plant(m, part, [pick(0.8, 0.3, 0.2)], 2, 7)
    plant(m, part, [pick(0.5, 0.2, 0.667)], 0, 12)         # touches colours 1 and 2
    plant(m, part, [pick(0.0, 0.0, 1.0)], 0, 6)            # domain corner
    x, y, z = cells(m, 12).T
    part[(x < 3) & (y < 3) & (z < 3)] = 2
    plant(m, part, [pick(0.2, 0.2, 0.5), pick(0.8, 0.8, 0.5)], 3, 5)
    return m, part, 4


def _cascade6():
    """Colour 2 in two pieces (x cell 2, x cells 4-5) kept apart by a colour-0
    wall (x cell 3) that touches colour 2 only; colour 0's main piece is x
    cells 0-1; colour 1 is a corner of the second piece."""
    m = M.kuhn_cube(6)
    x, y, z = cells(m, 6).T
    part = np.full(m.ne, 2, np.int32)
    part[x <= 1] = 0
    part[x == 3] = 0
    part[(x >= 4) & (z == 5) & (y == 5)] = 1
    return m, part, 3


def _unset(first, second):
    """Two disjoint cubes; colour 0 is all of the small cube (a piece with no
    neighbour outside) and, in the large one, the two sides of a colour-1 wall."""
    small_first = first < second
    m, ne1 = two_cubes(first, second)
    big = M.kuhn_cube(max(first, second), seed=77 if small_first else 20250117)
    x = cells(big, max(first, second))[:, 0]
    part = np.zeros(m.ne, np.int32)
    wall = np.nonzero(x == 2)[0] + (ne1 if small_first else 0)
    part[wall] = 1
    return m, part, 2


def _random(n, ncol, seed):
    m = M.kuhn_cube(n)
    return m, np.random.default_rng(seed).integers(0, ncol, m.ne).astype(np.int32), ncol


def _interface6():
    """nprocs = 3, myrank = 1: own colours 1, 4, 7 among the marks 0..7 of 8
    z-slabs, with fragments of own and of foreign colours planted."""
    m = M.kuhn_cube(6)
    part = slabs(m, 8)
    rng = np.random.default_rng(5)
    for colour, size in [(1, 1), (4, 3), (7, 2), (1, 6), (4, 1), (7, 8), (0, 2), (2, 4), (3, 1), (5, 5)]:
        plant(m, part, rng.choice(m.ne, 6, replace=False), colour, size)
    return m, part, np.array([1, 4, 7], np.int32)


def wave_mesh():
    return M.read_medit(os.path.join(ROOT, "tests", "golden", "ref_inputs", "wave.0.mesh"))


def _wave(kind):
    m = wave_mesh()
    rng = np.random.default_rng(11)
    if kind == "random":
        return m, rng.integers(0, 4, m.ne).astype(np.int32), 4
    c = m.centroids()
    left = c[:, 0] < np.median(c[:, 0])
    part = np.zeros(m.ne, np.int32)
    for side, base in ((left, 0), (~left, 2)):
        part[side] = base + (c[side, 1] >= np.median(c[side, 1]))
    for colour in range(4):
        plant(m, part, rng.choice(m.ne, 10, replace=False), colour, 1)
        plant(m, part, rng.choice(m.ne, 6, replace=False), colour, 4)
        plant(m, part, rng.choice(m.ne, 3, replace=False), colour, 15)
    return m, part, 4


def case(name):
    """(mesh, part, colors_or_n, twin part, twin stats), computed once."""
    if name not in _cases:
        if name == "planted12":
            m, part, col = _planted12()
        elif name == "cascade6":
            m, part, col = _cascade6()
        elif name == "unset_small_first":
            m, part, col = _unset(3, 6)
        elif name == "unset_large_first":
            m, part, col = _unset(6, 3)
        elif name.startswith("random"):
            n, ncol, seed = (int(v) for v in name.split("_")[1:])
            m, part, col = _random(n, ncol, seed)
        elif name == "interface6":
            m, part, col = _interface6()
        elif name.startswith("wave_"):
            m, part, col = _wave(name[5:])
        else:
            raise KeyError(name)
        fpart, st = fix(m, part, col)
        part.setflags(write=False)
        fpart.setflags(write=False)
        _cases[name] = (m, part, col, fpart, st)
    return _cases[name]


RANDOM_CASES = [f"random_{n}_{ncol}_{seed}" for n in (4, 6) for ncol in (3, 5) for seed in (1, 2, 3, 4)]
