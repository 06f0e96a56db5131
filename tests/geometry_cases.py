"""Thin, far and graded images of one mesh (no tests here).

Every mesh the location is tested on elsewhere fills a near-cubical box of
size about 1 at the origin.  A ParMmg group is a sub-box of the scaled mesh
away from the origin, often a thin slab, and graded.  The cases here are
images of the jittered kuhn_cube(8) (3072 tets, 768 trias) and of its points:
new_points(8) (512 volume, 384 surface) plus 200 uniform volume points of
[-0.1, 1.1]^3 (half of them outside the mesh).

  base     the identity
  plate    diag(1, 1, 2^-8)
  rod      diag(2^16, 1, 1): both grid clamps are reached (4096 / 1024 cells)
  slab     diag(2^6, 1, 2^-4)
  tiny     2^-20 x, hausd scaled alike
  huge     2^12 x, hausd scaled alike
  corner   x / 8 + 0.875 (inexact: simply another mesh)
  graded   x^3 per axis (orientation kept; most grid cells are empty)

hausd: a power-of-two image scales the surface's normal distances by at least
its smallest factor, so hausd is 0.01 times that factor -- the plate is thinner
than 0.01, and with the unscaled value a point on one face would lie within
hausd of the opposite one; `corner` 0.01 / 8; `graded` keeps 0.01.
test_starts_cpu checks that these leave reference_locate nothing undecidable
on the oracle's answers.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from parmmg_amd import mesh as M

N = 8
POW2 = {"plate": (1.0, 1.0, 2.0 ** -8), "rod": (2.0 ** 16, 1.0, 1.0), "slab": (2.0 ** 6, 1.0, 2.0 ** -4),
        "tiny": (2.0 ** -20,) * 3, "huge": (2.0 ** 12,) * 3}
NAMES = ("base", "plate", "rod", "slab", "tiny", "huge", "corner", "graded")
ANISO = ("plate", "rod", "slab")            # volume points invariant
UNIFORM = ("tiny", "huge")                  # everything invariant
REFERENCED = ("base", "plate", "slab", "corner", "graded")     # inside reference_locate's absolute TOL


def image(name, x):
    x = np.asarray(x, np.float64)
    if name == "base":
        return x.copy()
    if name in POW2:
        return x * np.array(POW2[name])[None]
    if name == "corner":
        return x / 8.0 + 0.875
    if name == "graded":
        return x * x * x
    raise KeyError(name)


def hausd(name):
    if name in POW2:
        return 0.01 * min(POW2[name])
    return 0.01 / 8.0 if name == "corner" else 0.01


@functools.lru_cache(maxsize=None)
def base_points():
    """(x (1096, 3), tags): new_points(8), then 200 uniform volume points."""
    x, t = M.new_points(N)
    extra = np.random.default_rng(41).uniform(-0.1, 1.1, size=(200, 3))
    return (np.ascontiguousarray(np.concatenate([x, extra])),
            np.concatenate([t, np.zeros(len(extra), np.uint16)]).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, points, tags) of a geometry; the caller must not modify them."""
    m = M.kuhn_cube(N)
    x, t = base_points()
    xyz = image(name, m.xyz)
    xyz[0] = 0.0
    return dataclasses.replace(m, xyz=np.ascontiguousarray(xyz), hausd=hausd(name)), np.ascontiguousarray(image(name, x)), t


@functools.lru_cache(maxsize=None)
def references(name):
    """(volume_ref of the volume points, surface_ref of the surface points):
    the long-double tables, once per geometry, shared by the CPU and the GPU
    module and by every run mode."""
    import reference_locate as RL
    m, x, t = case(name)
    return RL.volume_ref(m, x[t == 0]), RL.surface_ref(m, x[t != 0])


def fields(m):
    """[shock tensor, scalar, vector] on the BASE coordinates of the vertices
    (the same values on every image: the invariance tests compare them bit
    for bit)."""
    b = M.kuhn_cube(N)
    assert b.np == m.np
    return [M.on_vertices(b, M.shock_metric), M.on_vertices(b, M.iso_metric), M.on_vertices(b, M.velocity)]


# ---- the invariances under a power-of-two image ---------------------------------------
#
# Under an axis-wise power-of-two map every term of a determinant scales by
# the same power of two, so every comparison of the location keeps its outcome
# and every barycentric its bits (no overflow, no underflow at these sizes).

@dataclasses.dataclass
class Run:
    sols: list
    elem: np.ndarray
    status: np.ndarray
    steps: np.ndarray
    edge: np.ndarray
    vertex: np.ndarray


def _bits(a, b):
    a = np.ascontiguousarray(a, np.float64).view(np.int64)
    b = np.ascontiguousarray(b, np.float64).view(np.int64)
    if a.shape[0] == 0:
        return np.ones(0, bool)
    return (a == b).reshape(a.shape[0], -1).all(axis=1)


def assert_volume_invariant(what, tags, base: Run, img: Run):
    """Axis-wise image: a volume point has the base run's elem and
    status != 0, a found one bit-identical fields.  (A not-found point's
    values are not compared: the nearest vertex is not affine-invariant.)"""
    vol = np.nonzero(np.asarray(tags) == 0)[0]
    assert np.array_equal(img.elem[vol], base.elem[vol]), (what, vol[img.elem[vol] != base.elem[vol]][:10])
    assert np.array_equal(img.status[vol] != 0, base.status[vol] != 0), what
    found = vol[base.status[vol] != 0]
    assert len(found) >= 600 and len(vol) - len(found) >= 50, what
    for k, (a, b) in enumerate(zip(img.sols, base.sols)):
        ok = _bits(a[found], b[found])
        assert ok.all(), (what, k, found[~ok][:10])


def assert_identical(what, idx, base: Run, img: Run, walk=True):
    """Uniform image: everything of the points idx is the base run's -- elem,
    signed status, steps, edge, vertex and every field bit for bit.  walk
    False leaves out what depends on the walk's path (the sign of a found
    status, steps), for points whose two walks started at different tets."""
    idx = np.asarray(idx)
    for f in ("elem", "edge", "vertex") + (("status", "steps") if walk else ()):
        a, b = getattr(img, f)[idx], getattr(base, f)[idx]
        assert np.array_equal(a, b), (what, f, idx[a != b][:10])
    assert np.array_equal(img.status[idx] != 0, base.status[idx] != 0), what
    for k, (a, b) in enumerate(zip(img.sols, base.sols)):
        ok = _bits(a[idx], b[idx])
        assert ok.all(), (what, k, idx[~ok][:10])
