"""The CPU twin of pmx_metis_graph (tests/c/metis_graph_ref.c) on its own: the
semantics of PMMG_graph_meshElts2metis / PMMG_computeWgt (reference
src/metis_pmmg.c:746-823, :280-301) against values worked out by hand and a
numpy derivation from the adjacency, and the binding's declarations."""
import math
import os
import re

import numpy as np

import metis_ref as R
from conftest import ROOT
from parmmg_amd import _native as N
from parmmg_amd import mesh as M


def two_tets():
    """Tets (1,2,3,4) and (2,3,4,5) sharing the face (2,3,4), whose three
    edges all have Euclidean length sqrt(2)."""
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float64)
    tet = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [2, 3, 4, 5]], np.int32)
    return M.from_tets(xyz, tet)


def test_two_tets_by_hand():
    m = two_tets()
    s2 = math.sqrt(2.0)
    # face 0 of tet 1 (opposite vertex 1) and face 3 of tet 2 (opposite vertex 5)
    assert list(m.adja[1:9]) == [4 * 2 + 3, 0, 0, 0, 0, 0, 0, 4 * 1 + 0]
    # h = 1: three lengths sqrt(2) > 1, res = 3 (1/sqrt(2) - 1), w = exp(28 (1 - 1/sqrt(2))) = 3644.6...
    g = R.graph(m, np.ones((6, 1)))
    assert list(g["xadj"]) == [0, 1, 2] and list(g["adjncy"]) == [1, 0] and g["n"] == 2
    assert np.allclose(g["len"][:, :3], s2, rtol=1e-15)
    w = math.exp(28.0 * (1.0 - 1.0 / s2))
    assert 3644 < w < 3645
    assert np.allclose(g["wgt"], w, rtol=1e-13) and list(g["iwgt"]) == [3644, 3644]
    # h = 4: lengths sqrt(2)/4 <= 1, res = 3 (sqrt(2)/4 - 1), exp(18.1) > 1000000: clamped
    g = R.graph(m, np.full((6, 1), 4.0))
    assert np.allclose(g["len"][:, :3], s2 / 4, rtol=1e-15)
    assert list(g["wgt"]) == [1000000.0, 1000000.0] and list(g["iwgt"]) == [1000000, 1000000]
    assert np.allclose(g["len"][:, 3], math.exp(28.0 * (1.0 - s2 / 4)), rtol=1e-13)
    # h = 0.25: lengths 4 sqrt(2) > 1, res = 3 (1/(4 sqrt(2)) - 1): both branches
    # give terms <= 0, a face far from unit lengths on either side is heavy
    g = R.graph(m, np.full((6, 1), 0.25))
    assert np.allclose(g["len"][:, 3], math.exp(28.0 * (1.0 - 1.0 / (4 * s2))), rtol=1e-13)
    assert list(g["iwgt"]) == [1000000, 1000000]
    # h = 1.4: lengths sqrt(2)/1.4 = 1.0102 > 1, w = exp(28 (1 - 1.4/sqrt(2))) = 1.32...: integer weight 1
    g = R.graph(m, np.full((6, 1), 1.4))
    assert np.allclose(g["wgt"], math.exp(28.0 * (1.0 - 1.4 / s2)), rtol=1e-12) and list(g["iwgt"]) == [1, 1]
    # varying sizes: h(3) = 2, else 1.  MMG5_lenedg_iso of (3,4) and (2,3) is
    # sqrt(2) / (h2 - h1) log(h2 / h1) = sqrt(2) log 2 (<= 1), of (2,4) sqrt(2)
    h = np.ones((6, 1))
    h[3] = 2.0
    g = R.graph(m, h)
    l = s2 * math.log(2.0)
    assert np.allclose(sorted(g["len"][0, :3]), sorted([l, l, s2]), rtol=1e-14)
    # MMG5_iarf[0] = {5, 4, 3}: edges (3,4), (2,4), (2,3) of tet (1,2,3,4), in this order
    assert np.allclose(g["len"][0, :3], [l, s2, l], rtol=1e-14)
    res = 2 * (l - 1.0) + (1.0 / s2 - 1.0)
    assert np.allclose(g["wgt"], math.exp(-28.0 * res / 3.0), rtol=1e-13)
    # no metric: PMMG_WGTVAL_HUGEINT
    g = R.graph(m, None)
    assert list(g["iwgt"]) == [1000000, 1000000]
    # the face list: 12 ie + 3 ifac (+ iloc, ignored); a boundary face has a weight too
    fw = R.face_weights(m, [12 * 1 + 0, 12 * 2 + 3 * 3 + 2, 12 * 1 + 3], h)
    assert fw[0] == g_w(m, h)[0] and fw[1] == g_w(m, h)[1] and 0.0 < fw[2] <= 1000000.0


def g_w(m, h):
    return R.graph(m, h)["wgt"]


def test_tensor_identity_equals_iso_one():
    """A unit tensor measures Euclidean lengths, as h = 1 does; with
    metRidTyp = 1 and every vertex a ridge point no vertex is left for the
    tet's mean metric: every length 0, res = -3, w = exp(28) clamped."""
    m = two_tets()
    met = np.tile(np.array([1.0, 0, 0, 1, 0, 1]), (6, 1))
    g = R.graph(m, met)
    assert np.allclose(g["wgt"], math.exp(28.0 * (1.0 - 1.0 / math.sqrt(2.0))), rtol=1e-13)
    tags = np.full(6, 2, np.uint16)          # MG_GEO
    g1 = R.graph(m, met, met_rid_typ=1, tags=tags)
    assert np.all(g1["len"][:, :3] == 0.0) and list(g1["iwgt"]) == [1000000, 1000000]
    # one ridge endpoint: it takes the mean of the others' metrics, here the same unit tensor
    tags[:] = 0
    tags[2] = 2
    g2 = R.graph(m, met, met_rid_typ=1, tags=tags)
    assert np.array_equal(g2["wgt"], g["wgt"])


def test_kuhn_structure_against_numpy():
    m = M.kuhn_cube(4)
    g = R.graph(m, weights=False)
    xadj, adjncy = R.numpy_graph(m)
    assert np.array_equal(g["xadj"], xadj) and np.array_equal(g["adjncy"], adjncy)
    assert g["n"] == 4 * m.ne - 2 * 6 * 4 * 4        # every boundary face is one entry less


def test_graph_is_symmetric():
    m = M.kuhn_cube(4)
    g = R.graph(m, R.iso_sizes(m, 4))
    src = np.repeat(np.arange(m.ne), np.diff(g["xadj"]))
    fwd = set(zip(src.tolist(), g["adjncy"].tolist()))
    assert len(fwd) == g["n"]                         # no repeated entry
    assert fwd == {(b, a) for a, b in fwd}
    # ... but the weights are not: the two tets see the same three edges, in
    # another order of summation at most
    w = {(a, b): x for a, b, x in zip(src.tolist(), g["adjncy"].tolist(), g["wgt"].tolist())}
    assert all(abs(w[(a, b)] - w[(b, a)]) <= 1e-12 * w[(a, b)] for a, b in fwd)


def test_issue_input_statistics():
    """The iso case of the GPU tests is what the issue says it is: lengths on
    both sides of 1, a tenth of the weights clamped, nothing borderline."""
    m = M.kuhn_cube(6)
    g = R.graph(m, R.iso_sizes(m, 6))
    L = g["len"][:, :3]
    assert g["n"] == 4752 and m.ne == 1296
    assert 0.31 < L.min() < 0.33 and 3.17 < L.max() < 3.19
    assert 0.60 < (L <= 1.0).mean() < 0.62
    assert 0.09 < (g["wgt"] >= 1000000.0).mean() < 0.10
    assert len(np.unique(g["iwgt"])) == 1799
    assert not R.borderline(g["len"][:, 3]).any()


def test_binding_declares_the_graph_entry_points():
    text = open(os.path.join(ROOT, "include", "pmx_transfer.h")).read()
    for sym in ("pmx_metis_graph", "pmx_face_weights"):
        assert sym in N.SIGNATURES and re.search(r"\b" + sym + r"\s*\(", text)
    from parmmg_amd.transfer import Transfer
    assert callable(Transfer.metis_graph) and callable(Transfer.face_weights)
