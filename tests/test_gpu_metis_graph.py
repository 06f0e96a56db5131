"""pmx_metis_graph / pmx_face_weights on the GPU against the CPU twin
(tests/c/metis_graph_ref.c): PMMG_graph_meshElts2metis and PMMG_computeWgt
(reference src/metis_pmmg.c:746-823, :280-301).

xadj / adjncy are exact.  The lengths are the reference's bit for bit (the
library restates glibc's log1p), so exp's argument is too; the device
library's exp and glibc's may differ in the last ulp, which changes an integer
weight only where the weight before the clamp is within an ulp of an integer
or of the clamp.  Entries within 1e-9 (relative) of one -- a classification
threshold, about 1e6 times the possible difference, not a tolerance -- are
"borderline": they may differ by 1 and may be at most 0.1 % of the entries.
Every other integer weight is equal.  The double weights of pmx_face_weights
are compared within 4 ulp: identical exp arguments, <= 1 ulp per exp, carried
1:1 by the reciprocal plus its own rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metis_ref as R
from conftest import ROOT
from helpers import cube_surface
from parmmg_amd import _native as N
from parmmg_amd import mesh as M
from parmmg_amd.transfer import Transfer

pytestmark = pytest.mark.gpu

SENT = -77
GEO, REQ, NOM, CRN = 2, 4, 8, 32
IARF = np.array([[5, 4, 3], [5, 1, 2], [4, 2, 0], [3, 0, 1]])

_cache = {}


def case(name):
    """Meshes, metrics and twin results shared by the tests (computed once)."""
    if name not in _cache:
        if name == "iso6":
            m = M.kuhn_cube(6)
            met = R.iso_sizes(m, 6)
        elif name == "ani6":
            m = M.kuhn_cube(6)
            met = R.rotated_tensor(m, 6)
        else:
            raise KeyError(name)
        _cache[name] = (m, met, R.graph(m, met))
    return _cache[name]


def ridge_tags(m, seed=3):
    """Ridge points on the x < 0.4 slab, some of them singular or
    non-manifold (not ridge points for MMG5_lenedg_ani)."""
    rng = np.random.default_rng(seed)
    tags = np.zeros(m.np + 1, np.uint16)
    slab = np.nonzero(m.xyz[:, 0] < 0.4)[0]
    slab = slab[slab > 0]
    tags[slab] = GEO
    extra = rng.choice(slab, size=len(slab) // 6, replace=False)
    tags[extra[: len(extra) // 3]] |= REQ
    tags[extra[len(extra) // 3: 2 * len(extra) // 3]] |= NOM
    tags[extra[2 * len(extra) // 3:]] |= CRN
    return tags


def raw_call(tr, ne, cap, weights=True, count_only=False, met_rid_typ=0):
    """pmx_metis_graph on sentinel-filled arrays of 4 ne + 8 ints: (return
    value, nadjncy, xadj, adjncy, adjwgt)."""
    xadj = np.full(ne + 1, SENT, np.int32)
    adjncy = np.full(4 * ne + 8, SENT, np.int32)
    adjwgt = np.full(4 * ne + 8, SENT, np.int32)
    n = C.c_int64(-1)
    p = lambda a: a.ctypes.data_as(N.i32ptr)
    r = tr.lib.pmx_metis_graph(tr.ctx, met_rid_typ, p(xadj), None if count_only else p(adjncy),
                               p(adjwgt) if weights and not count_only else None, cap, C.byref(n))
    return r, n.value, xadj, adjncy, adjwgt


def assert_weights(iw, g, frac=0.001):
    """The comparison rule of the module docstring; returns the borderline count."""
    b = R.borderline(g["len"][:, 3])
    assert b.mean() <= frac, f"{b.sum()} borderline entries of {len(b)}"
    d = iw.astype(np.int64) - g["iwgt"]
    print(f"entries {len(b)} borderline {int(b.sum())} differing {int((d != 0).sum())}")
    assert np.all(d[~b] == 0), f"{(d[~b] != 0).sum()} non-borderline weights differ, max {np.abs(d[~b]).max()}"
    assert np.all(np.abs(d[b]) <= 1)
    return int(b.sum())


# ---- 1. structure ----------------------------------------------------------------

@pytest.mark.parametrize("n,ne,nadj", [(6, 1296, 4752), (12, 10368, None)])
@pytest.mark.parametrize("variant", ["adja", "device_adja", "shuffle"])
def test_structure(transfer, n, ne, nadj, variant):
    m = M.kuhn_cube(n)
    if variant == "shuffle":
        m, _ = M.numbering(m, "shuffle")
    assert m.ne == ne
    xadj, adjncy = R.numpy_graph(m)
    if nadj is not None:
        assert len(adjncy) == nadj and 4 * ne - nadj == 432
    transfer.upload_background(m, [R.iso_sizes(m, n)], 0, adja=variant != "device_adja")
    xa, ad, aw = transfer.metis_graph()
    assert xa.dtype == np.int32 and ad.dtype == np.int32 and aw.dtype == np.int32
    assert np.array_equal(xa, xadj) and np.array_equal(ad, adjncy) and len(aw) == len(ad)
    # count only: xadj and nadjncy, the other arrays untouched
    r, cnt, xa2, ad2, aw2 = raw_call(transfer, ne, 4 * ne, count_only=True)
    assert r == 1 and cnt == len(adjncy) and np.array_equal(xa2, xadj)
    assert np.all(ad2 == SENT) and np.all(aw2 == SENT)
    # weights off: adjwgt untouched, nothing past nadjncy written
    r, cnt, xa3, ad3, aw3 = raw_call(transfer, ne, 4 * ne, weights=False)
    assert r == 1 and cnt == len(adjncy) and np.array_equal(ad3[:cnt], adjncy)
    assert np.all(ad3[cnt:] == SENT) and np.all(aw3 == SENT)
    xa4, ad4, aw4 = transfer.metis_graph(weights=False)
    assert aw4 is None and np.array_equal(ad4, adjncy)


# ---- 2. iso weights --------------------------------------------------------------

def test_iso_weights(transfer):
    m, met, g = case("iso6")
    L = g["len"][:, :3]
    # the input exercises both length branches and the clamp
    assert (L <= 1.0).mean() >= 0.05 and (L > 1.0).mean() >= 0.05
    assert (g["wgt"] >= 1000000.0).mean() >= 0.05 and (g["wgt"] < 1000000.0).mean() >= 0.05
    transfer.upload_background(m, [met], 0)
    xa, ad, aw = transfer.metis_graph()
    assert np.array_equal(xa, g["xadj"]) and np.array_equal(ad, g["adjncy"])
    assert aw.min() >= 1 and aw.max() == 1000000
    assert assert_weights(aw, g) == 0          # this input has no borderline entry


# ---- 3. tensor metric ------------------------------------------------------------

def test_tensor_weights(transfer):
    m, met, g = case("ani6")
    L = g["len"][:, :3]
    assert (L <= 1.0).mean() >= 0.2 and (L > 1.0).mean() >= 0.2
    assert (g["wgt"] >= 1000000.0).mean() >= 0.05
    assert np.abs(met[1:, [1, 2, 4]]).min() > 0.0            # a full tensor, not a diagonal one
    transfer.upload_background(m, [met], 0)
    xa, ad, aw = transfer.metis_graph()
    assert np.array_equal(ad, g["adjncy"])
    assert_weights(aw, g)


# ---- 4. metRidTyp = 1 ------------------------------------------------------------

def test_ridge_storage(transfer):
    m, met, g0 = case("ani6")
    tags = ridge_tags(m)
    g1 = R.graph(m, met, met_rid_typ=1, tags=tags)
    assert (g1["iwgt"] != g0["iwgt"]).mean() > 0.05, "the ridge points must change weights"
    transfer.upload_background(m, [met], 0)
    with pytest.raises(RuntimeError, match="point tags"):
        transfer.metis_graph(met_rid_typ=1)
    transfer.upload_point_tags(tags)
    xa, ad, aw = transfer.metis_graph(met_rid_typ=1)
    assert np.array_equal(ad, g1["adjncy"])
    assert_weights(aw, g1)
    # metRidTyp = 0 ignores the tags
    assert_weights(transfer.metis_graph(met_rid_typ=0)[2], g0)
    with pytest.raises(RuntimeError, match="metRidTyp"):
        transfer.metis_graph(met_rid_typ=2)


def test_iso_metric_ignores_met_rid_typ(transfer):
    m, met, g = case("iso6")
    transfer.upload_background(m, [met], 0)
    a0 = transfer.metis_graph(met_rid_typ=0)
    a1 = transfer.metis_graph(met_rid_typ=1)              # no tags needed
    transfer.upload_point_tags(ridge_tags(m))
    a2 = transfer.metis_graph(met_rid_typ=1)
    for a in (a1, a2):
        assert all(np.array_equal(x, y) for x, y in zip(a0, a))


# ---- 5. surface data -------------------------------------------------------------

def test_surface_data(transfer):
    m, met, g = case("ani6")
    tags, surf, _ = cube_surface(m)
    transfer.upload_background(m, [met], 0)
    plain = transfer.metis_graph()
    transfer.upload_point_tags(tags)
    transfer.upload_surface(surf)
    xa, ad, aw = transfer.metis_graph()
    assert np.array_equal(xa, plain[0]) and np.array_equal(ad, plain[1])
    # entries whose face holds an xTetra edge tagged MG_BDY
    ne = m.ne
    k = np.repeat(np.arange(1, ne + 1), np.diff(xa))
    f = np.nonzero(m.adja[1:4 * ne + 1].reshape(ne, 4) != 0)[1]
    et = (surf["xtag"][surf["xt"][k]] & 16) != 0                    # (n, 6)
    tagged = et[np.arange(len(k))[:, None], IARF[f]].any(1)
    assert 0.01 < tagged.mean() < 0.5
    assert np.array_equal(aw[~tagged], plain[2][~tagged])
    assert np.all(aw[tagged] >= 1) and np.all(aw[tagged] <= 1000000)
    assert (aw[tagged] != plain[2][tagged]).any(), "the surface lengths must bite"
    fw = transfer.face_weights(12 * k[tagged] + 3 * f[tagged])
    assert np.all(np.isfinite(fw)) and np.all(fw >= 1.0) and np.all(fw <= 1000000.0)
    # dropped again: back to the plain graph
    transfer.upload_surface(None)
    assert np.array_equal(transfer.metis_graph()[2], plain[2])


# ---- 6. no metric ----------------------------------------------------------------

def test_no_metric(transfer):
    m = M.kuhn_cube(6)
    transfer.upload_background(m, [M.on_vertices(m, M.level_set)], -1)
    xa, ad, aw = transfer.metis_graph()
    assert len(aw) == 4752 and np.all(aw == 1000000)
    assert np.all(transfer.face_weights([12, 12 * m.ne + 9]) == 1000000.0)


# ---- 7. face weights -------------------------------------------------------------

def test_face_weights(transfer):
    m, met, g = case("iso6")
    rng = np.random.default_rng(17)
    k = rng.integers(1, m.ne + 1, 200)
    f = rng.integers(0, 4, 200)
    faces = (12 * k + 3 * f + rng.integers(0, 3, 200)).astype(np.int32)      # + iloc, ignored
    bdy = m.adja[4 * (k - 1) + 1 + f] == 0
    assert 5 <= bdy.sum() <= 195
    ref = R.face_weights(m, faces, met)
    transfer.upload_background(m, [met], 0)
    w = transfer.face_weights(faces)
    ulp = np.abs(w - ref) / np.spacing(ref)
    print(f"face weights: max {ulp.max():.1f} ulp, {int((ulp > 0).sum())} of {len(ulp)} differ")
    assert ulp.max() <= 4.0
    assert (ref >= 1000000.0).any() and (ref < 1000000.0).any()
    for bad in (11, 12 * (m.ne + 1), -5):
        with pytest.raises(RuntimeError, match="outside"):
            transfer.face_weights([12, bad])
    assert len(transfer.face_weights([])) == 0


# ---- 8. resident path ------------------------------------------------------------

def test_promoted_group(transfer):
    """After a step and pmx_promote_background the promoted group's graph is
    that of a fresh upload of the same mesh and metric."""
    m1 = M.kuhn_cube(5, seed=101)
    m2 = M.kuhn_cube(6, seed=202)
    x2 = m2.xyz[1:].copy()
    onb = np.any((x2 == 0.0) | (x2 == 1.0), axis=1)
    t2 = np.where(onb, M.TAG_BDY, 0).astype(np.uint16)
    tets2 = m2.tet.copy() - 1
    tets2[0] = -1
    tr = Transfer(0)
    ref = Transfer(0)
    try:
        for metric in (R.iso_sizes(m1, 6), R.rotated_tensor(m1, 6)):
            tr.upload_background(m1, [metric], 0)
            tr.upload_points(x2, t2, tets2)
            tr.run()
            r2 = tr.download()
            tr.promote_background(m2, r2.sols, adja=False)
            a = tr.metis_graph()
            met2 = np.zeros((m2.np + 1, metric.shape[1]))
            met2[1:] = r2.sols[0]
            ref.upload_background(m2, [met2], 0)
            b = ref.metis_graph()
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert len(np.unique(a[2])) > 100
    finally:
        tr.close()
        ref.close()


# ---- 9. edges and refusals -------------------------------------------------------

def test_small_meshes(transfer):
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float64)
    one = M.from_tets(xyz[:5], np.array([[0, 0, 0, 0], [1, 2, 3, 4]], np.int32))
    transfer.upload_background(one, [np.ones((5, 1))], 0)
    xa, ad, aw = transfer.metis_graph()
    assert list(xa) == [0, 0] and len(ad) == 0 and len(aw) == 0
    two = M.from_tets(xyz, np.array([[0, 0, 0, 0], [1, 2, 3, 4], [2, 3, 4, 5]], np.int32))
    transfer.upload_background(two, [np.ones((6, 1))], 0)
    xa, ad, aw = transfer.metis_graph()
    assert list(xa) == [0, 1, 2] and list(ad) == [1, 0] and list(aw) == [3644, 3644]
    k1 = M.kuhn_cube(1)
    met = R.iso_sizes(k1, 1)
    g = R.graph(k1, met)
    transfer.upload_background(k1, [met], 0)
    xa, ad, aw = transfer.metis_graph()
    assert k1.ne == 6 and np.array_equal(xa, g["xadj"]) and np.array_equal(ad, g["adjncy"])
    assert_weights(aw, g, frac=1.0)


def test_refusals(transfer):
    tr = Transfer(0)
    try:
        with pytest.raises(RuntimeError, match="upload a group first"):
            tr.metis_graph()
        with pytest.raises(RuntimeError, match="upload a group first"):
            tr.face_weights([12])
        assert tr.kernel_ms(8) == -1.0
    finally:
        tr.close()
    m, met, g = case("iso6")
    transfer.upload_background(m, [met], 0)
    n = g["n"]
    r, cnt, xa, ad, aw = raw_call(transfer, m.ne, n - 1)
    assert r == 0 and cnt == n
    assert b"nadjncy" in transfer.lib.pmx_last_error(transfer.ctx)
    assert np.all(xa == SENT) and np.all(ad == SENT) and np.all(aw == SENT)
    r, cnt, xa, ad, aw = raw_call(transfer, m.ne, n)                 # exactly enough
    assert r == 1 and cnt == n and np.array_equal(ad[:n], g["adjncy"]) and np.all(ad[n:] == SENT)
    assert np.all(aw[n:] == SENT)
    assert transfer.kernel_ms(8) > 0.0
    assert transfer.kernel_ms(8) == pytest.approx(sum(transfer.kernel_ms(w) for w in (9, 10, 11)))
    # a deleted tet: the reference wants a packed mesh
    md = M.Mesh(m.xyz, m.tet.copy(), m.adja, m.tria, m.adjt)
    md.tet[77, 0] = 0
    transfer.upload_background(md, [met], 0)
    with pytest.raises(RuntimeError, match="deleted tet"):
        transfer.metis_graph()


# ---- 10. C driver ----------------------------------------------------------------

DEMO_SRC = os.path.join(ROOT, "tests", "c", "metis_graph_demo.c")
DEMO_BIN = os.path.join(ROOT, "tests", "c", "_build", "metis_graph_demo")


def build_demo() -> str:
    os.makedirs(os.path.dirname(DEMO_BIN), exist_ok=True)
    gen = os.path.join(ROOT, "parmmg_amd", "csrc", "meshgen.c")
    deps = [DEMO_SRC, gen, os.path.join(ROOT, "include", "pmx_transfer.h"), N.LIB_PATH]
    if (not os.path.exists(DEMO_BIN)
            or any(os.path.getmtime(DEMO_BIN) < os.path.getmtime(d) for d in deps if os.path.exists(d))):
        subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-std=c99", "-I",
                        os.path.join(ROOT, "include"), DEMO_SRC, gen, "-o", DEMO_BIN, "-L",
                        os.path.dirname(N.LIB_PATH), "-lpmx_transfer",
                        "-Wl,-rpath," + os.path.dirname(N.LIB_PATH), "-lm"], check=True)
    return DEMO_BIN


def fnv(a) -> int:
    h = 1469598103934665603
    for x in np.asarray(a, np.int32).view(np.uint32).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_driver(transfer):
    r = subprocess.run([build_demo()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "graph ok" in r.stdout
    m, met, g = case("iso6")
    transfer.upload_background(m, [met], 0)
    xa, ad, aw = transfer.metis_graph()
    line = f"graph ne={m.ne} nadjncy={len(ad)} xadj={fnv(xa):016x} adj={fnv(ad):016x} wgt={fnv(aw):016x}"
    assert line in r.stdout, r.stdout
