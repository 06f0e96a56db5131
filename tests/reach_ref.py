"""The CPU twin of pmx_check_reachability / pmx_moveifc_fix / pmx_moveifc_reach
(tests/c/reach_ref.c) through ctypes, an independent numpy check of its result
and the cases the reachability tests share (test infrastructure).  The twin is
UNPINNED: Mmg is absent, so the reference file it restates cannot be built
here."""
import ctypes as C
import os
import subprocess

import numpy as np

import contiguity_ref as R
from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "reach_ref.c")
LIB = os.path.join(ROOT, "tests", "c", "_build", "libreach_ref.so")

NPROCS, MYRANK = 3, 1
COLORS = np.array([1, 4, 7], np.int32)          # nprocs * i + myrank, i < 3
UNSET = -1

_lib = None


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("nseeds", "nreached", "nreached_tets", "nunreached", "nmerged",
                                         "nmerged_tets", "nrescanned", "ncannot", "counter", "fix_nmerged",
                                         "fix_nmerged_tets", "fix_ncannot", "nchained", "nbeside_reached")]


# the fields pmx_reach_stats shares with the twin
REACH_FIELDS = ("nseeds", "nreached", "nreached_tets", "nunreached", "nmerged", "nmerged_tets", "nrescanned",
                "ncannot", "counter")


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
        l.rcr_fix.restype = None
        l.rcr_fix.argtypes = [i64, vp, vp, vp, C.POINTER(C.c_int), C.c_int, vp, C.POINTER(Stats)]
        l.rcr_reach.restype = C.c_int
        l.rcr_reach.argtypes = [i64, vp, vp, vp, C.POINTER(C.c_int), i64, vp, vp, C.POINTER(Stats)]
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _dict(st):
    return {f: getattr(st, f) for f, _ in st._fields_}


class Twin:
    """The reference's state over both calls: mark, flag (1-based) and base."""

    def __init__(self, m, mark):
        self.m = m
        self.adja = np.ascontiguousarray(m.adja, np.int32)
        self.mk = np.zeros(m.ne + 1, np.int32)
        self.mk[1:] = mark
        self.flag = np.zeros(m.ne + 1, np.int32)
        self.base = C.c_int(0)
        self.st = Stats()

    @property
    def mark(self):
        return self.mk[1:].copy()

    def fix(self, colors=COLORS):
        col = np.ascontiguousarray(colors, np.int32)
        lib().rcr_fix(self.m.ne, _p(self.adja), _p(self.mk), _p(self.flag), C.byref(self.base), len(col), _p(col),
                      C.byref(self.st))
        return self.mark, _dict(self.st)

    def reach(self, face_index1, color_in):
        """False when an entry is out of range; counter goes on from the fix's."""
        fi = np.ascontiguousarray(face_index1, np.int32)
        cin = np.ascontiguousarray(color_in, np.int32)
        ok = lib().rcr_reach(self.m.ne, _p(self.adja), _p(self.mk), _p(self.flag), C.byref(self.base), len(fi),
                             _p(fi) if len(fi) else None, _p(cin) if len(fi) else None, C.byref(self.st))
        return bool(ok), self.mark, _dict(self.st)


def run(m, mark, face_index1, color_in, colors=COLORS):
    """Fix, then the check: the fixed marks, the fix's counter, the flags the
    fix left (nonzero / zero), the final marks and the twin's stats."""
    t = Twin(m, mark)
    fixed, fst = t.fix(colors)
    flagged = t.flag[1:] != 0
    ok, out, st = t.reach(face_index1, color_in)
    assert ok
    for a in (fixed, flagged, out):
        a.setflags(write=False)
    return {"fixed": fixed, "fix_counter": fst["counter"], "fix_stats": fst, "flagged": flagged, "mark": out,
            "stats": st, "all_flagged": bool(np.all(t.flag[1:] != 0))}


# ---- the entries of the face communicator ------------------------------------------------

def zrel(m):
    z = m.centroids()[:, 2]
    return (z - z.min()) / (z.max() - z.min())


def entries(m, thick):
    """The boundary tets of the bottom layer (relative centroid height below
    `thick`; the neighbour is rank 0) and of the top one (rank 2), each with
    its first boundary face: (face_index1, rank_out)."""
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) // 4
    z = zrel(m)
    fi, rank = [], []
    for lay, r in ((z < thick, 0), (z > 1.0 - thick, 2)):
        for k in np.nonzero(lay & (nb == 0).any(1))[0]:
            f = int(np.argmax(nb[k] == 0))
            fi.append(12 * (k + 1) + 3 * f)
            rank.append(r)
    return np.array(fi, np.int32), np.array(rank, np.int32)


def honest(mark, fi, rank):
    """What a neighbour reports for an entry: the tet's colour when that is one
    of the neighbour's, nothing otherwise."""
    c = np.asarray(mark)[fi // 12 - 1]
    return np.where(c % NPROCS == rank, c, UNSET).astype(np.int32)


def slab_marks(m, colours):
    """8 z-slabs, slab i with colours[i]."""
    return np.asarray(colours, np.int32)[R.slabs(m, 8)]


# ---- independent of the twin ---------------------------------------------------------------

def numpy_check(m, mark, fi, cin, colors=COLORS):
    """Every piece of a colour that is not the rank's either holds the tet of
    an entry that received this colour, or has no neighbour outside ("cannot
    merge").  Returns the number of the latter."""
    ncomp, lab = R.numpy_labels(m, mark)
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) // 4
    labz = np.concatenate([[0], lab])
    closed_tet = ((nb == 0) | (labz[nb] == lab[:, None])).all(1)
    seeded = set()
    for f, c in zip(fi, cin):
        if c != UNSET and mark[f // 12 - 1] == c:
            seeded.add(int(lab[f // 12 - 1]))
    ncannot = 0
    for l in np.unique(lab[~np.isin(mark, colors)]):
        if int(l) in seeded:
            continue
        assert closed_tet[lab == l].all(), f"the piece of tet {l} (colour {mark[l - 1]}) is foreign and unreached"
        ncannot += 1
    return ncannot


# ---- the cases (shared by the CPU and the GPU tests) ---------------------------------------

FOREIGN_SLABS = [0, 0, 1, 4, 4, 7, 2, 2]            # colour 0 on the bottom interface, colour 2 on the top one


def _pick(m, x, y, z):
    return R.nearest(m, x, y, z)


def _local4():
    m = M.kuhn_cube(4)
    mark = slab_marks(m, [1, 1, 4, 4, 4, 7, 7, 7])
    R.plant(m, mark, [_pick(m, 0.3, 0.3, 0.8)], 1, 3)         # the fix has work, the check has none
    R.plant(m, mark, [_pick(m, 0.7, 0.6, 0.1)], 7, 1)
    return m, mark, 0.25, "honest"


def _reached6():
    m = M.kuhn_cube(6)
    return m, slab_marks(m, FOREIGN_SLABS), 1 / 6, "honest"


def _fragments6():
    """Foreign single tets, pairs and blobs in the interior of case reached6;
    one blob lies across the boundary of colours 4 and 7."""
    m, mark, thick, _ = _reached6()
    mark = mark.copy()
    R.plant(m, mark, [_pick(m, 0.3, 0.3, 0.45), _pick(m, 0.7, 0.2, 0.7)], 3, 1)
    R.plant(m, mark, [_pick(m, 0.6, 0.6, 0.4), _pick(m, 0.2, 0.8, 0.55)], 5, 2)
    R.plant(m, mark, [_pick(m, 0.8, 0.8, 0.5)], 6, 9)
    R.plant(m, mark, [_pick(m, 0.5, 0.2, 0.625)], 8, 12)      # touches colours 4 and 7
    R.plant(m, mark, [_pick(m, 0.4, 0.7, 0.3)], 0, 4)         # the bottom slab's colour, away from it
    return m, mark, thick, "honest"


def _nested(n, seed, nfrag, thick):
    """Foreign blobs carved into foreign blobs: unreached lists whose first
    outside neighbour lies in another unreached list."""
    m = M.kuhn_cube(n)
    mark = slab_marks(m, FOREIGN_SLABS)
    rng = np.random.default_rng(seed)
    interior = np.nonzero((zrel(m) > 0.3) & (zrel(m) < 0.7))[0]
    for s in rng.choice(interior, nfrag, replace=False):
        blob = R.plant(m, mark, [s], int(rng.choice([0, 3, 5, 6])), int(rng.integers(4, 12)))
        R.plant(m, mark, [blob[-1]], int(rng.choice([0, 2, 3, 8])), int(rng.integers(1, 4)))
        R.plant(m, mark, [blob[len(blob) // 2]], int(rng.choice([0, 5, 6])), 1)
    return m, mark, thick, "honest"


def _beside6():
    """Fragments on top of the reached bottom slab, colour 0 among them: a
    list that joined an unflagged colour-0 list is met again beside the slab."""
    m = M.kuhn_cube(6)
    mark = slab_marks(m, FOREIGN_SLABS)
    rng = np.random.default_rng(BESIDE_SEED)
    z = zrel(m)
    above = np.nonzero((z > 0.25) & (z < 0.36))[0]            # the cells that touch the slab from above
    for s in rng.choice(above, 10, replace=False):
        blob = R.plant(m, mark, [s], int(rng.choice([3, 6])), int(rng.integers(3, 8)))
        R.plant(m, mark, [blob[-1]], 0, int(rng.integers(1, 4)))
    return m, mark, 1 / 6, "honest"


def _two_cubes():
    """The small cube wholly of a foreign colour nobody reports: it has no
    neighbour outside and stays."""
    m, ne1 = R.two_cubes(3, 6)
    big = M.kuhn_cube(6, seed=77)
    mark = np.full(m.ne, 3, np.int32)
    mark[ne1:] = slab_marks(big, FOREIGN_SLABS)
    return m, mark, 1 / 6, "honest"


def _random(n, seed):
    m = M.kuhn_cube(n)
    return m, np.random.default_rng(seed).integers(0, 8, m.ne).astype(np.int32), 1 / n, f"random{seed}"


def _wave():
    m = R.wave_mesh()
    mark = slab_marks(m, FOREIGN_SLABS)
    rng = np.random.default_rng(11)
    for colour in (0, 2, 3, 5, 6, 1, 4):
        R.plant(m, mark, rng.choice(m.ne, 8, replace=False), colour, 1)
        R.plant(m, mark, rng.choice(m.ne, 5, replace=False), colour, 4)
        R.plant(m, mark, rng.choice(m.ne, 3, replace=False), colour, 15)
    return m, mark, 1 / 8, "honest"


NESTED_SEED, BESIDE_SEED = 3, 2
_builders = {
    "local4": _local4, "reached6": _reached6, "fragments6": _fragments6,
    "nested6": lambda: _nested(6, NESTED_SEED, 12, 1 / 6), "beside6": _beside6, "two_cubes": _two_cubes,
    "wave": _wave,
}
_cases = {}


def case(name):
    """{"m", "mark0" (before the fix), "fi", "rank", "cin", and the twin's run}
    computed once.  name: a builder, optionally with a variant of the colours
    received after '@': other (the bottom neighbour reports colour 3), unset
    (nobody reports anything), dup (every fifth entry twice, and every seventh
    entry a colour its tet does not have), small_unset (two_cubes: nothing for
    the entries of the small cube)."""
    if name not in _cases:
        base, _, variant = name.partition("@")
        if base.startswith("random_"):
            n, seed = (int(v) for v in base.split("_")[1:])
            m, mark, thick, how = _random(n, seed)
        else:
            m, mark, thick, how = _builders[base]()
        fi, rank = entries(m, thick)
        fixed = Twin(m, mark).fix()[0]
        if how == "honest":
            cin = honest(fixed, fi, rank)
        else:
            rng = np.random.default_rng(100 + int(how[6:]))
            cin = rng.integers(-1, 9, len(fi)).astype(np.int32)
        if variant == "other":
            cin = np.where(rank == 0, 3, UNSET).astype(np.int32)
        elif variant == "unset":
            cin = np.full(len(fi), UNSET, np.int32)
        elif variant == "dup":
            fi = np.concatenate([fi, fi[::5]])
            cin = np.concatenate([cin, cin[::5]])
            cin[::7] = 6
        elif variant == "small_unset":
            cin[fi // 12 <= M.kuhn_cube(3).ne] = UNSET
        elif variant:
            raise KeyError(name)
        mark.setflags(write=False)
        d = {"m": m, "mark0": mark, "fi": fi, "rank": rank, "cin": cin}
        d.update(run(m, mark, fi, cin))
        _cases[name] = d
    return _cases[name]


RANDOM_CASES = [f"random_{n}_{seed}" for n in (4, 6) for seed in (1, 2, 3, 4)]
CASES = ["local4", "reached6", "reached6@other", "reached6@unset", "fragments6", "nested6", "beside6", "two_cubes@small_unset",
         "fragments6@dup"] + RANDOM_CASES + ["wave"]
