"""GPU: every device tensor path on generic tensors, against the oracle bit for
bit AND against the independent long-double reference (tests/reference_hp.py).

The other suites feed the tensor kernels mesh.shock_metric, diag(1/h^2) or
ridge rows: tensors whose three diagonal entries are bitwise equal and whose
three off-diagonal entries are too, so a kernel that reads m[2] for m[4]
returns the same bits.  helpers.generic_tensor has six different entries
everywhere (test_reference_cpu.test_mutations: any swap of two components
moves the results by 1e6 tolerances).

Every item asserts device == oracle by the project's rules (compare_volume /
compare_exact, sums within 1e-12, everything else exact).  Where the reference
defines the operation -- interpolation, quality, classic-storage length -- the
item also asserts device == reference within 8 x the noise floor (the largest
float64 / long double deviation of the reference on the same inputs; never
derived from the oracle's or the kernel's error), counts and histograms
exactly.  The curved surface lengths and the ridge storage are compared with
the oracle only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reference_hp as R
from conftest import REF_INPUTS
from helpers import (bits_equal, compare_exact, compare_volume, cube_surface, generic_tensor, generic_tensor_edges,
                     graded_iso_scaled, ridge_tags, split_partitions, unit_box)
from oracle import oracle as O
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from test_gpu_stats import assert_len_equal, assert_len_exact, assert_qual_equal

pytestmark = pytest.mark.gpu

SENT = R.SENT


def second_tensor(x):
    """Another generic field: the first one on permuted, shrunk coordinates."""
    return 0.37 * generic_tensor(0.15 + 0.7 * x[:, [2, 0, 1]])


def positive_vector(m):
    return np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), 2.0 + np.cos(2.0 * m.xyz[1:])]))


def sent(n, sols):
    return [np.full((n, s.shape[1]), SENT) for s in sols]


@pytest.fixture(scope="module")
def cube6():
    """kuhn_cube(6) and its new points, plus surface points on the edge and at
    a vertex of boundary trias (the metric is then interpolated along the
    edge / copied), points on an interior face and an interior edge of the
    background and two points outside the cube."""
    m = M.kuhn_cube(6)
    x, t = M.new_points(6)
    border = [0.5 * (m.xyz[m.tria[k, 1]] + m.xyz[m.tria[k, 2]]) for k in (17, 140, 301)]
    border += [0.25 * m.xyz[m.tria[77, 0]] + 0.75 * m.xyz[m.tria[77, 1]], m.xyz[m.tria[200, 2]].copy()]
    x = np.concatenate([x, np.array(border)])
    t = np.concatenate([t, np.full(len(border), M.TAG_BDY, np.uint16)])
    adj = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4)
    inner = np.nonzero((adj > 0).all(axis=1))[0] + 1            # tets without a boundary face
    extra = []
    for k in inner[[5, 111, 402]]:
        extra.append(m.xyz[m.tet[k, 1:]].mean(axis=0))          # on the face opposite vertex 0
    for k in inner[[37, 250]]:
        extra.append(0.5 * (m.xyz[m.tet[k, 0]] + m.xyz[m.tet[k, 2]]))
    extra += [np.array([1.03, 0.41, 0.57]), np.array([0.33, -0.02, 0.71])]
    x = np.concatenate([x, np.array(extra)])
    t = np.concatenate([t, np.zeros(len(extra), np.uint16)])
    return m, x, t


@pytest.fixture(scope="module")
def wave():
    m = M.read_medit(os.path.join(REF_INPUTS, "wave.0.mesh"))
    return m, M.on_vertices(m, unit_box(generic_tensor)), graded_iso_scaled(m)


def step(tr, m, x, t, sols, imet, flags=0, hsiz=0.0):
    tr.upload_background(m, sols, imet)
    tr.upload_points(x, t)
    tr.run(flags=flags, hsiz=hsiz, record_starts=True)
    r = tr.download(init=sent(len(x), sols))
    e, v = tr.border()
    return r, tr.starts(), e, v


def check_oracle(m, x, t, sols, imet, r, starts, edge, vert, replace=None):
    """The step against the oracle in device semantics.  replace: {solution:
    rows} the oracle does not compute (the constant-size metric)."""
    o = O.Oracle(m)
    outs, elem, st, _, e, v = o.interp(x, t, sols, imet=imet, init=sent(len(x), sols), fresh=True,
                                       start_vol=starts, start_bdy=starts)
    for k, rows in (replace or {}).items():
        outs[k] = rows
    bdy = np.nonzero((t & M.TAG_BDY) != 0)[0]
    compare_exact((r.sols, r.elem, r.status, edge, vert), (outs, elem, st, e, v), bdy, len(sols))
    c = compare_volume(o, x, t, (r.sols, r.elem, r.status), (outs, elem, st), sols)
    assert c["same"] + c["ties"] == c["nvol"]
    return c


def check_reference(m, x, t, sols, imet, r, edge, vert, label, only=None):
    """The step against the reference, at the device's own elements."""
    bdy = (t & M.TAG_BDY) != 0
    written = []
    for k, s in enumerate(sols):
        if only is not None and k not in only:
            continue
        floor, err, w = R.interp_errors(m, x, t, r.elem, r.status, s, r.sols[k], edge=edge, vert=vert,
                                        metric=k == imet)
        written.append(w)
        for cls, sel in (("volume", ~bdy[w]), ("surface", bdy[w])):
            if sel.any():
                print(f"{label} sol {k} size {s.shape[1]} {cls}: floor {float(floor[sel].max()):.3g} "
                      f"device {float(err[sel].max()):.3g}")
                assert err[sel].max() <= 8 * floor[sel].max(), (label, k, cls)
    return written


# ---- the step, LAYOUT_ANI --------------------------------------------------------

@pytest.mark.parametrize("mode", ["plain", "refwalk", "noties"])
def test_step_metric_alone(transfer, cube6, mode):
    """The metric alone (imet = 0): interp_layout<LAYOUT_ANI>, the surface
    points' interp_bar<3> / interp_tria, and the fallback's closest-element
    interpolation for the two points outside."""
    m, x, t = cube6
    sols = [M.on_vertices(m, generic_tensor)]
    flags = {"plain": 0, "refwalk": N.RUN_REFERENCE_WALK, "noties": N.RUN_NO_INLINE_TIES}[mode]
    r, starts, edge, vert = step(transfer, m, x, t, sols, 0, flags)
    assert (r.status[-2:] == 0).all() and np.all(r.status[:-2] != 0)
    assert ((t & M.TAG_BDY) != 0).sum() == 216 + 5 and not np.any(r.sols[0] == SENT)
    assert (edge != -1).sum() >= 4 and (vert != -1).sum() >= 1          # the border cases of the surface path
    c = check_oracle(m, x, t, sols, 0, r, starts, edge, vert)
    print(mode, c)
    w, = check_reference(m, x, t, sols, 0, r, edge, vert, mode)
    assert w.all()


# ---- the step, LAYOUT_GEN --------------------------------------------------------

def test_step_four_fields(transfer, cube6):
    """scalar + metric + vector + a second tensor, imet = 1: interp_bar<4> /
    interp_bar<3> on every size."""
    m, x, t = cube6
    sols = [M.on_vertices(m, M.graded_iso_metric(6)), M.on_vertices(m, generic_tensor), positive_vector(m),
            M.on_vertices(m, second_tensor)]
    r, starts, edge, vert = step(transfer, m, x, t, sols, 1)
    check_oracle(m, x, t, sols, 1, r, starts, edge, vert)
    for w in check_reference(m, x, t, sols, 1, r, edge, vert, "gen"):
        assert w.all()


def test_step_planted_rows(transfer, cube6):
    """The metric of generic_tensor_edges: the diagonal branch of the
    inversion on either side of its threshold, and the rows of the points
    whose element holds the singular vertex left untouched."""
    m, x, t = cube6
    met, planted = generic_tensor_edges(m, M.on_vertices(m, generic_tensor))
    sols = [M.on_vertices(m, M.graded_iso_metric(6)), met]
    r, starts, edge, vert = step(transfer, m, x, t, sols, 1)
    check_oracle(m, x, t, sols, 1, r, starts, edge, vert)
    _, w = check_reference(m, x, t, sols, 1, r, edge, vert, "planted")
    vol = (t & M.TAG_BDY) == 0
    sing = np.zeros(len(x), bool)
    sing[vol] = np.isin(m.tet[r.elem[vol]], planted["singular"]).any(axis=1)
    assert np.array_equal(~w, sing) and 1 <= sing.sum() <= 0.05 * len(x)
    assert (r.sols[1][sing] == SENT).all() and not (r.sols[0] == SENT).any()
    for name in ("zero", "below", "above"):
        hit = np.zeros(len(x), bool)
        hit[vol] = np.isin(m.tet[r.elem[vol]], planted[name]).any(axis=1)
        assert hit.sum() >= 1, name


def test_step_constant_size(transfer, cube6):
    """hsiz > 0: the size-6 constant metric (k_const_metric) next to a generic
    tensor field, which is still interpolated."""
    m, x, t = cube6
    sols = [M.on_vertices(m, generic_tensor), M.on_vertices(m, second_tensor)]
    hsiz = 0.05
    r, starts, edge, vert = step(transfer, m, x, t, sols, 0, hsiz=hsiz)
    const = np.zeros((len(x), 6))
    O.load().orc_constant_size(len(x), 6, hsiz, const.ctypes.data)
    assert bits_equal(r.sols[0], const).all()
    assert np.all(R.full(r.sols[0], np.float64) == np.eye(3) / (hsiz * hsiz))
    check_oracle(m, x, t, sols, 0, r, starts, edge, vert, replace={0: const})
    w, = check_reference(m, x, t, sols, -1, r, edge, vert, "hsiz", only=(1,))
    assert w.all()


# ---- quality ---------------------------------------------------------------------

def check_quality(q, qo, P, M4, ridge, label):
    assert np.array_equal(q.view(np.int64)[1:], qo.view(np.int64)[1:]), "quality not bit-equal to the oracle's"
    ref, floor, err = R.quality_errors(P, M4, q[1:], ridge)
    print(f"{label}: floor {float(floor.max()):.3g} device {float(err.max()):.3g}")
    assert err.max() <= 8 * floor.max()
    return ref, 8 * float(floor.max())


def test_quality_wave(transfer, wave):
    """k_qual<ANI> with the plain mean (tetra_qual, qualhisto(INQUA))."""
    m, met, _ = wave
    T = m.tet[1:]
    transfer.upload_background(m, [met], 0)
    transfer.upload_point_tags(None)
    q = transfer.tetra_qual(m.ne, 0)
    qo = O.tetra_qual(m, met)
    ref, tol = check_quality(q, qo, m.xyz[T], met[T], None, "wave quality")
    h = transfer.qualhisto(N.INQUA)
    assert_qual_equal(h, O.qualhisto(m, qo))
    R.check_qual_stats(h, ref, T, None, tol)


def test_quality_ridge(transfer):
    """cube 7 with ridge points: qualhisto(OUTQUA) and tetra_qual(met_rid_typ=1),
    the mean metric without the non-singular ridge points."""
    m = M.kuhn_cube(7)
    tags = ridge_tags(m)
    met = M.on_vertices(m, generic_tensor)
    T = m.tet[1:]
    transfer.upload_background(m, [met], 0)
    transfer.upload_point_tags(tags)
    q = transfer.tetra_qual(m.ne, 1)
    qo = O.tetra_qual(m, met, tags=tags, met_rid_typ=1)
    ridge = R.is_ridge(tags)[T]
    ref, tol = check_quality(q, qo, m.xyz[T], met[T], ridge, "cube7 ridge quality")
    assert (ref == 0).sum() > 0 and (ridge.any(axis=1) & ~ridge.all(axis=1)).sum() > 0
    h = transfer.qualhisto(N.OUTQUA)
    ho = O.qualhisto(m, qo, tags=tags)
    assert ho["nrid"] > 0
    assert_qual_equal(h, ho)
    R.check_qual_stats(h, ref, T, tags, tol)
    transfer.upload_point_tags(None)


def test_new_mesh_quality(transfer):
    """new_mesh_qual after the LAYOUT_ANI step and new_mesh_qual_synced: the
    reference evaluated on the device's own interpolated metric."""
    m = M.kuhn_cube(6)
    sols = [M.on_vertices(m, generic_tensor)]
    new = M.kuhn_cube(6, seed=77)
    x = new.xyz[1:].copy()
    t = np.zeros(len(x), np.uint16)
    tv = new.tet.copy()
    tv[0] = 0
    transfer.upload_background(m, sols, 0)
    transfer.upload_point_tags(None)
    transfer.upload_points(x, t, tets_mmg=tv)
    transfer.run()
    r = transfer.download()
    assert np.all(r.status != 0) and np.isfinite(r.sols[0]).all()
    met = np.concatenate([np.zeros((1, 6)), r.sols[0]])
    T = new.tet[1:]
    q = transfer.new_mesh_qual(None, N.INQUA)
    qo = O.tetra_qual(new, met)
    check_quality(q, qo, new.xyz[T], met[T], None, "new mesh quality")
    qs = transfer.new_mesh_qual_synced(met)
    qso = O.tetra_qual(new, met, tags=np.zeros(new.np + 1, np.uint16), met_rid_typ=1)
    check_quality(qs, qso, new.xyz[T], met[T], np.zeros((new.ne, 4), bool), "new mesh quality, synced")


# ---- lengths ---------------------------------------------------------------------

def check_lengths(L, Lo, m, met, tags=None):
    if met.shape[1] == 6:
        assert_len_exact(L, Lo)
    else:
        assert_len_equal(L, Lo)
    ed, ref, floor = R.length_reference(m, met, tags)
    return R.check_len_stats(L, ed, ref, 8 * floor)


@pytest.mark.parametrize("metric", ["ani", "iso"])
def test_lengths_wave(transfer, wave, metric):
    """k_prilen on ~50 batches of 256 tets with varying vertex valence."""
    m, met, iso = wave
    mm = met if metric == "ani" else iso
    transfer.upload_background(m, [mm], 0)
    transfer.upload_point_tags(None)
    s = check_lengths(transfer.prilen(), O.prilen(m, mm), m, mm)
    assert all(s["hl"]), s["hl"]


_PB_SCRIPT = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import generic_tensor, graded_iso_scaled, unit_box
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer
m = M.read_medit(os.path.join(sys.argv[1], "tests", "golden", "ref_inputs", "wave.0.mesh"))
tr = Transfer(0)
out = []
for mm in (M.on_vertices(m, unit_box(generic_tensor)), graded_iso_scaled(m)):
    tr.upload_background(m, [mm], 0)
    out.append(tr.prilen())
print(json.dumps(out))
'''


def test_lengths_wave_wide_index(wave):
    """The 64-bit-index instantiations of k_prilen (PMX_PRILEN_WIDE=1, read
    once per process: a child process)."""
    m, met, iso = wave
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PMX_PRILEN_WIDE="1")
    p = subprocess.run([sys.executable, "-c", _PB_SCRIPT, root], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for L, mm in zip(got, (met, iso)):
        check_lengths(L, O.prilen(m, mm), m, mm)


def test_lengths_ridge(transfer):
    """cube 7 with ridge points: the tets of 4 ridge points are left out."""
    m = M.kuhn_cube(7)
    tags = ridge_tags(m)
    met = M.on_vertices(m, generic_tensor)
    transfer.upload_background(m, [met], 0)
    transfer.upload_point_tags(tags)
    check_lengths(transfer.prilen(), O.prilen(m, met, tags=tags), m, met, tags)
    transfer.upload_point_tags(None)


@pytest.mark.parametrize("once", [0, 1])
def test_lengths_partitions(transfer, once):
    """k_prilen_par on the two halves of cube 6: the oracle for the parallel
    edges (their lengths are curved surface lengths), the reference for the
    number of edges each rank counts."""
    full = M.kuhn_cube(6)
    parts, nshared = split_partitions(full)
    assert nshared > 0
    for rank, (mr, glob, par) in enumerate(parts):
        met = M.on_vertices(mr, generic_tensor)
        p = dict(par, myrank=rank, owner=np.zeros(len(par["a"]), np.int32), exact_once=once)
        transfer.upload_background(mr, [met], 0)
        transfer.upload_point_tags(None)
        L = transfer.prilen(par=p)
        assert_len_exact(L, O.prilen(mr, met, par=p))
        ed = R.unique_edges(mr.tet[1:])
        assert L["ned"] + L["nullEdge"] == len(ed) - (nshared if once and rank == 1 else 0)


@pytest.mark.parametrize("mrt", [0, 1])
def test_lengths_surface(transfer, mrt):
    """cube_surface with the generic tensor off the ridge rows: the curved
    surface lengths and the ridge storage, against the oracle only."""
    m = M.kuhn_cube(7)
    tags, surf, met = cube_surface(m, noise=0.08, base=generic_tensor)
    transfer.upload_background(m, [met], 0)
    transfer.upload_point_tags(tags)
    transfer.upload_surface(surf)
    L = transfer.prilen(met_rid_typ=mrt)
    Lo = O.prilen(m, met, tags=tags, met_rid_typ=mrt, surface=surf)
    assert_len_exact(L, Lo)
    assert sum(1 for h in Lo["hl"] if h) >= 4
    transfer.upload_surface(None)
    transfer.upload_point_tags(None)
