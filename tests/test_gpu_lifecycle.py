"""A context gives back everything it allocated: one cycle through every
module that owns device or pinned memory, three times over, leaves
pmx_debug_live_allocations() where it was, and the third cycle's results are
bit-equal to the first's.

The session-wide `transfer` fixture stays alive throughout, so the counter is
compared with its value before the cycle, not with zero."""
import numpy as np
import pytest

from helpers import bits_equal, cube_case, split_partitions
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

NCUBE = 8


@pytest.fixture(scope="module")
def case():
    m, x, t, sols = cube_case(NCUBE, metric="iso", surface=True)
    sols = sols[:3]                                    # the metric and two fields
    extra = M.on_vertices(m, M.velocity)
    tets = M.new_point_tets(NCUBE, x, t)
    # helpers.split_partitions' two sides as a part array, one tet of side 0
    # moved deep into side 1: fix_contiguity has a component to merge
    parts, _ = split_partitions(m)
    c = m.centroids()
    part = (c[:, 0] >= 0.5).astype(np.int32)
    assert [int((part == r).sum()) for r in (0, 1)] == [p[0].ne for p in parts]
    part[np.argmax(c[:, 0])] = 0
    groups = []
    for n, seed in ((5, 1), (6, 2)):
        gm, gx, gt, gs = cube_case(n, metric="iso", seed_pts=seed)
        groups.append((gm, gx, gt, gs))
    return m, x, t, sols, extra, tets, part, groups


def live(lib):
    return lib.pmx_debug_live_allocations()


def cycle(case):
    """Every array the cycle downloads, and the counter before and after."""
    m, x, t, sols, extra, tets, part, groups = case
    lib = N.load()
    before = live(lib)
    out = []
    tr = Transfer(0)
    try:
        tr.upload_background(m, sols, 0, adja=False)   # the device builds the adjacency
        tr.upload_points(x, t, tets_mmg=tets)
        tr.run(flags=N.RUN_EAGER_DOWNLOAD)
        r = tr.download()
        assert np.all(r.status != 0), "points not located"
        out += r.sols + [r.elem, r.status]
        out += tr.interp_more([extra])
        xadj, adjncy, adjwgt = tr.metis_graph()
        out += [xadj, adjncy, adjwgt]
        ncomp, counts, label = tr.contiguity(part, 2)
        assert ncomp == 3
        fixed, st = tr.fix_contiguity(part, 2)
        assert st["nmerged"] == 1
        out += [counts, label, fixed]
        plan = tr.split_groups(fixed, 2)
        g0 = tr.split_fetch(0)
        out += [plan["sizes"], plan["tet_new"], g0["tetra_v"][1:], g0["adja"][1:], g0["xyz"][1:]]
        out += [s[1:] for s in g0["sols"]]
        out.append(tr.build_adja(m.tet, m.np)[1:])
        gl = []
        for gm, gx, gt, gs in groups:
            xyz1 = np.concatenate([np.zeros((1, 3)), gx])
            tag1 = np.concatenate([np.zeros(1, np.uint16), gt])
            gl.append(dict(old_mesh=gm, old_met=gs[0], old_fields=gs[1:], xyz=xyz1, tags=tag1,
                           met=np.zeros((len(xyz1), 1)),
                           fields=[np.zeros((len(xyz1), s.shape[1])) for s in gs[1:]], hsiz=0.0))
        assert tr.interp_metrics_and_fields(gl, input_met=1) == 1   # two groups: the peer context
        for g in gl:
            out += [g["met"][1:]] + [f[1:] for f in g["fields"]]
        assert live(lib) > before
    finally:
        tr.close()
    return out, before, live(lib)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(bits_equal(a.reshape(len(a), -1), b.reshape(len(b), -1)).all()) if a.size else True
    return bool(np.array_equal(a, b))


def test_three_cycles_leave_nothing_behind(transfer, case):
    first = None
    for k in range(3):
        out, before, after = cycle(case)
        assert after == before, f"cycle {k + 1}: {after - before} allocations outlive their context"
        if first is None:
            first = out
    assert len(out) == len(first)
    for i, (a, b) in enumerate(zip(first, out)):
        assert same(a, b), f"downloaded array {i} of cycle 3 differs from cycle 1"
