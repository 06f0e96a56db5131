"""The CPU twin of the group split (tests/c/split_ref.c, a restatement of the
reference's PMMG_split_eachGrp, src/grpsplit_pmmg.c:1267-1445) checked by
properties, so that the device (tests/test_gpu_split.py) is compared against
something that has itself been checked; and the library's split surface."""
import ctypes
import os

import numpy as np
import pytest

import split_ref as S
from parmmg_amd import _native
from parmmg_amd import mesh as M

IDIR = S.IDIR


def _cases():
    m3, m6 = M.kuhn_cube(3), M.kuhn_cube(6)
    rnd = S.fix_empty(np.random.default_rng(7).integers(0, 5, m6.ne), 5)
    w = S.wave_mesh()
    return {"slabs2": (m3, S.slabs(m3, 2), 2), "slabs3": (m3, S.slabs(m3, 3), 3),
            "slabs8": (m6, S.slabs(m6, 8), 8), "boustrophedon": (m6, S.boustrophedon(m6, 6), 2),
            "random5": (m6, rnd, 5), "modulo1000": (m6, S.modulo_parts(m6.ne, 1000), 1000),
            "wave4": (w, S.x_slabs(w, 4), 4)}


CASES = _cases()
_splits = {}


def split_of(name):
    if name not in _splits:
        m, part, ngrp = CASES[name]
        _splits[name] = S.split(m, part, ngrp)
    return CASES[name] + (_splits[name],)


def old_nb(m):
    """(ne, 4) old neighbour tets (0 none) and their faces."""
    a = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4)
    return a // 4, a % 4


@pytest.mark.parametrize("name", list(CASES))
def test_tets_points_and_connectivity(name):
    m, part, ngrp, sp = split_of(name)
    seen = []
    for g, grp in enumerate(sp["groups"]):
        told, tv, pold = grp["tet_old"], grp["tetra_v"], grp["point_old"]
        assert np.array_equal(sp["sizes"][g], [len(told), len(pold), len(grp["face_index1"]), len(grp["node_index1"])])
        # tet coverage: ascending, this part's tets, tet_new the inverse
        assert np.all(np.diff(told) > 0) and np.all(part[told - 1] == g)
        assert np.array_equal(sp["tet_new"][told - 1], np.arange(1, len(told) + 1))
        seen.append(told)
        # connectivity round trip
        assert np.array_equal(pold[tv[1:] - 1], m.tet[told])
        # first visit: scanned tet by tet, slot by slot, new ids appear as 1, 2, 3, ...
        flat = tv[1:].ravel()
        first = np.sort(np.unique(flat, return_index=True)[1])
        assert np.array_equal(flat[first], np.arange(1, len(pold) + 1))
        assert len(np.unique(pold)) == len(pold)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(1, m.ne + 1))


@pytest.mark.parametrize("name", list(CASES))
def test_adjacency(name):
    m, part, ngrp, sp = split_of(name)
    nb, _ = old_nb(m)
    for g, grp in enumerate(sp["groups"]):
        told, tv = grp["tet_old"], grp["tetra_v"]
        neg = len(told)
        a = grp["adja"][1:4 * neg + 1].reshape(neg, 4)
        onb = nb[told - 1]
        same = (onb != 0) & (part[np.maximum(onb, 1) - 1] == g)
        assert np.array_equal(a != 0, same)                  # non-zero exactly where the old neighbour stays
        j, f = np.nonzero(a)
        j2, f2 = a[j, f] // 4 - 1, a[j, f] % 4
        assert np.array_equal(told[j2], onb[j, f])           # the same neighbour as before
        assert np.array_equal(a[j2, f2], 4 * (j + 1) + f)    # symmetric
        va = np.sort(tv[1:][j[:, None], IDIR[f]], axis=1)
        vb = np.sort(tv[1:][j2[:, None], IDIR[f2]], axis=1)
        assert np.array_equal(va, vb)                        # the same face on both sides


@pytest.mark.parametrize("name", list(CASES))
def test_face_communicator(name):
    m, part, ngrp, sp = split_of(name)
    nb, _ = old_nb(m)
    ncut = int(((nb != 0) & (part[np.maximum(nb, 1) - 1] != part[:, None])).sum())
    assert sp["int_face_nitem"] * 2 == ncut
    where = {}
    for g, grp in enumerate(sp["groups"]):
        i1, i2 = grp["face_index1"], grp["face_index2"]
        assert np.all(np.diff(i1 // 3) > 0)                  # (local tet, face) order
        for e in range(len(i1)):
            j, f, iploc = i1[e] // 12, (i1[e] % 12) // 3, i1[e] % 3
            k = grp["tet_old"][j - 1]
            assert nb[k - 1, f] != 0 and part[nb[k - 1, f] - 1] != g
            face = frozenset(m.tet[k][IDIR[f]])
            where.setdefault(int(i2[e]), []).append((g, face, m.tet[k][IDIR[f][iploc]]))
    assert sorted(where) == list(range(sp["int_face_nitem"]))
    for pos, sides in where.items():
        assert len(sides) == 2
        (g1, face1, v1), (g2, face2, v2) = sides
        assert g1 != g2 and face1 == face2 and v1 == v2
    # positions are handed out along the lists in the order the groups are filled
    i2 = sp["groups"][0]["face_index2"]
    assert np.array_equal(i2, np.arange(len(i2)))


@pytest.mark.parametrize("name", list(CASES))
def test_node_communicator_manifold(name):
    m, part, ngrp, sp = split_of(name)
    value, count, total = {}, {}, 0
    member = {}
    for g, grp in enumerate(sp["groups"]):
        for v in grp["point_old"]:
            member.setdefault(int(v), []).append(g)
        n1, n2 = grp["node_index1"], grp["node_index2"]
        assert len(np.unique(n1)) == len(n1)
        total += len(n1)
        for lp, val in zip(n1, n2):
            v = int(grp["point_old"][lp - 1])
            assert value.setdefault(v, int(val)) == val      # one value per vertex
            count[v] = count.get(v, 0) + 1
    shared = {v for v, gs in member.items() if len(gs) >= 2}
    assert set(count) == shared                              # exactly the vertices of several groups
    assert all(count[v] == len(member[v]) for v in shared)   # once in each of them
    assert len(set(value.values())) == len(value)            # distinct vertices, distinct values
    assert sp["int_node_nitem"] == total


def test_old_communicators_pass_through():
    m = M.kuhn_cube(4)
    sp = S.split(m, S.slabs(m, 2), 2, data=(m.xyz, []))
    g0 = sp["groups"][0]
    m0 = S.group_mesh(g0)
    assert np.array_equal(m0.adja, g0["adja"])               # from_tets rebuilds what the split kept
    x = m0.centroids()[:, 0]
    part2 = (x >= np.median(x)).astype(np.int32)
    comm = S.group_comm(g0, sp)
    sp2 = S.split(m0, part2, 2, comm)
    # old faces: same position and starting vertex, re-based to the new local tets
    old = {}
    for i1, i2 in zip(g0["face_index1"], g0["face_index2"]):
        old[(i1 // 12, (i1 % 12) // 3)] = (i1 % 3, i2)
    seen, newpos = set(), []
    for g, grp in enumerate(sp2["groups"]):
        for i1, i2 in zip(grp["face_index1"], grp["face_index2"]):
            key = (int(grp["tet_old"][i1 // 12 - 1]), int((i1 % 12) // 3))
            if key in old:
                assert (i1 % 3, i2) == old[key]
                seen.add(key)
            else:
                newpos.append(int(i2))
    assert seen == set(old)
    nnew = len(newpos) // 2
    assert nnew > 0 and sorted(newpos) == sorted(2 * list(range(sp["int_face_nitem"], sp["int_face_nitem"] + nnew)))
    assert sp2["int_face_nitem"] == sp["int_face_nitem"] + nnew
    # old nodes keep their value in every new group that holds them
    oldval = dict(zip(g0["node_index1"].tolist(), g0["node_index2"].tolist()))
    for grp in sp2["groups"]:
        got = dict(zip(grp["point_old"][grp["node_index1"] - 1].tolist(), grp["node_index2"].tolist()))
        for v in grp["point_old"].tolist():
            if v in oldval:
                assert got[v] == oldval[v]
    # the counter counts appends: every entry of both new lists
    assert sp2["int_node_nitem"] == sp["int_node_nitem"] + sum(len(g["node_index1"]) for g in sp2["groups"])


def test_non_manifold_order_dependence():
    """Two blocks glued at one vertex; block A in two slabs that both touch it.
    The vertex lies on no cut face of B's group (B is cut from nothing).  The
    reference's rule: a group lists a vertex without a cut face of its own only
    when an earlier-filled group has given it a value."""
    m, ne_a, corner = S.glued_cubes()
    nb, _ = old_nb(m)
    assert not np.any((nb[:ne_a] > ne_a)) and not np.any((nb[ne_a:] != 0) & (nb[ne_a:] <= ne_a))
    for ids, listed in (((0, 2, 1), True), ((1, 2, 0), False)):
        part = S.glued_parts(m, ne_a, ids)
        holds = np.any(m.tet[1:] == corner, axis=1)
        assert set(part[holds]) == set(ids)                  # all three groups hold the corner
        sp = S.split(m, part, 3)
        gb = sp["groups"][ids[2]]
        lp = int(np.nonzero(gb["point_old"] == corner)[0][0]) + 1
        assert len(gb["face_index1"]) == 0                   # B has no cut face at all
        assert (lp in gb["node_index1"].tolist()) == listed
        if listed:
            assert gb["node_index1"].tolist() == [lp]
            g0 = sp["groups"][ids[0]]
            l0 = int(np.nonzero(g0["point_old"] == corner)[0][0]) + 1
            assert gb["node_index2"][0] == g0["node_index2"][g0["node_index1"].tolist().index(l0)]
        for g in ids[:2]:                                    # A's slabs list it either way
            grp = sp["groups"][g]
            assert int(np.nonzero(grp["point_old"] == corner)[0][0]) + 1 in grp["node_index1"].tolist()


def test_library_surface():
    names = ("pmx_split_groups", "pmx_split_fetch", "pmx_split_release")
    assert os.path.exists(_native.LIB_PATH), "libpmx_transfer.so not built"
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert all(n in _native.SIGNATURES for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "pmx_transfer.h")).read()
    assert all(f"int {n}(" in header for n in names)
