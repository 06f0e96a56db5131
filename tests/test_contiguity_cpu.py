"""The CPU twin of pmx_contiguity / pmx_fix_contiguity (tests/c/contiguity_ref.c)
on its own: its breadth-first counts against the literal restatement of the
reference's two sweep counters (src/metis_pmmg.c:312-392, 446-529) and against
an independent numpy min-label iteration; FIX against
cases worked out by hand on chains of tets; that every planted case of the GPU
tests exercises the path it is named for; and the binding's declarations."""
import os
import re

import numpy as np
import pytest

import contiguity_ref as R
from conftest import ROOT
from parmmg_amd import _native as N
from parmmg_amd import mesh as M


def chains(*lengths):
    """Disjoint chains of tets: a chain of n tets has the vertices p..p+n+2 on
    the moment curve and the tets (i, i+1, i+2, i+3), consecutive ones sharing
    the face (i+1, i+2, i+3).  Tets are numbered chain after chain."""
    xyz, tet = [[0.0, 0.0, 0.0]], [[0, 0, 0, 0]]
    for c, n in enumerate(lengths):
        p = len(xyz)
        for i in range(n + 3):
            t = 1.0 + i
            xyz.append([t + 100.0 * c, t * t, t * t * t])
        for i in range(n):
            tet.append([p + i, p + i + 1, p + i + 2, p + i + 3])
    return M.from_tets(np.array(xyz), np.array(tet, np.int32))


def test_chain_adjacency():
    m = chains(3, 1)
    nb = m.adja[1:17].reshape(4, 4) // 4
    # tet k's neighbour through the face opposite its first vertex is k + 1,
    # through the face opposite its last vertex k - 1
    assert [list(r) for r in nb] == [[2, 0, 0, 0], [3, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 0]]


def partitions():
    """(name, mesh, part or None, nparts) of every case the tests count on."""
    out = []
    for n, k in ((6, 3), (12, 8)):
        m = M.kuhn_cube(n)
        out.append((f"slabs{k}_{n}", m, R.slabs(m, k), k))
    m12 = M.kuhn_cube(12)
    out.append(("snake12", m12, R.boustrophedon(m12, 12), 2))
    out.append(("one_colour12", m12, None, 1))
    for name in ["planted12", "cascade6", "unset_small_first", "unset_large_first", "interface6", "wave_bisect",
                 "wave_random"] + R.RANDOM_CASES:
        m, part, col, fpart, _ = R.case(name)
        out.append((name, m, part, 8))
        out.append((name + "_fixed", m, fpart, 8))
    m2, _ = R.two_cubes(3, 4)
    out.append(("two_cubes", m2, None, 1))
    return out


def test_counts_three_ways():
    """Breadth-first search, the reference's sweeps and the numpy iteration
    agree on the number of components, per part and in all, and on the labels."""
    for name, m, part, nparts in partitions():
        ncomp, counts, label = R.components(m, part, nparts)
        n_np, lab_np = R.numpy_labels(m, part)
        assert ncomp == n_np and np.array_equal(label, lab_np), name
        if part is None:
            assert R.sweep_group(m) == ncomp, name
        else:
            last, sc = R.sweep_parts(m, part, nparts)
            assert np.array_equal(sc, counts) and last == counts[-1], name
            assert counts.sum() == ncomp, name       # every mark of these cases lies in 0..7
        # the label is the smallest tet of the component
        assert np.all(label <= np.arange(1, m.ne + 1)) and np.all(label[label - 1] == label), name


def test_clean_and_snake_counts():
    m = M.kuhn_cube(6)
    assert R.components(m, R.slabs(m, 3), 3)[:2][0] == 3
    assert R.sweep_group(m) == 1
    m2, ne1 = R.two_cubes(3, 4)
    n, _, label = R.components(m2)
    assert n == 2 and R.sweep_group(m2) == 2 and set(label) == {1, ne1 + 1}
    m12 = M.kuhn_cube(12)
    snake = R.boustrophedon(m12, 12)
    n, counts, _ = R.components(m12, snake, 2)
    assert n == 2 and list(counts) == [1, 1]
    # a path: far more label-propagation sweeps than a slab needs
    xadj, adjncy = R.numpy_graph(m12)
    on = np.nonzero(snake == 1)[0]
    dist = np.full(m12.ne, -1)
    dist[on[0]] = 0
    front = [on[0]]
    while front:
        nxt = []
        for k in front:
            for j in adjncy[xadj[k]:xadj[k + 1]]:
                if snake[j] == 1 and dist[j] < 0:
                    dist[j] = dist[k] + 1
                    nxt.append(j)
        front = nxt
    assert dist[on].min() >= 0 and dist.max() > 300, dist.max()


# ---- FIX by hand ------------------------------------------------------------------

def test_fix_tie_later_piece_loses():
    """Colour 0 = {1, 2} and {4, 5}: equal sizes, the later list merges (into
    colour 1, not yet processed: the counter goes down by its length)."""
    m = chains(7)
    part, st = R.fix(m, np.array([0, 0, 1, 0, 0, 1, 1], np.int32), 2)
    assert list(part) == [0, 0, 1, 1, 1, 1, 1]
    # colour 0: 2 + 2 - 2; colour 1: one list of 5
    assert st == dict(ncomp=4, nmerged=1, nmerged_tets=2, ncannot=0, counter=7)


def test_fix_swap_and_counter():
    """Colour 0 = {1} then {3, 4}: the later list is strictly longer, so the
    main list {1} merges (into colour 1, unprocessed: counter - 1) and {3, 4}
    becomes main.  Colour 1 is then {1, 2} and {5, 6, 7}: {1, 2} merges into
    tet 3's colour 0, already processed: the counter stays."""
    m = chains(7)
    part, st = R.fix(m, np.array([0, 1, 0, 0, 1, 1, 1], np.int32), 2)
    assert list(part) == [0, 0, 0, 0, 1, 1, 1]
    # colour 0: 1 + 2 - 1 = 2; colour 1: 2 + 3 = 5, nothing subtracted
    assert st == dict(ncomp=4, nmerged=2, nmerged_tets=3, ncannot=0, counter=7)
    # the other order of colours: colour 1 = {2} and {5, 6, 7}; {2} merges into
    # tet 3 (face 0 comes before face 3), colour 0, unprocessed: counter - 1;
    # colour 0 is then one list {1, 2, 3, 4}
    part, st = R.fix(m, np.array([0, 1, 0, 0, 1, 1, 1], np.int32), [1, 0])
    assert list(part) == [0, 0, 0, 0, 1, 1, 1]
    assert st == dict(ncomp=4, nmerged=1, nmerged_tets=1, ncannot=0, counter=1 + 3 - 1 + 4)


def test_fix_unset_main_keeps_its_place():
    """Colour 0 = the lone tet 1 (no neighbour at all), {2, 3} and {5, 6, 7}:
    both later lists are longer than main, main cannot merge and stays main,
    so neither of them is compared with the other and nothing moves."""
    m = chains(1, 6)
    p0 = np.array([0, 0, 0, 1, 0, 0, 0], np.int32)
    part, st = R.fix(m, p0, 2)
    assert list(part) == list(p0)
    assert st == dict(ncomp=4, nmerged=0, nmerged_tets=0, ncannot=2, counter=7)


def test_fix_unset_next():
    """Colour 0 = the closed chain {1, 2, 3} and the lone tet 4: the later,
    smaller list has no neighbour outside and cannot merge."""
    m = chains(3, 1)
    part, st = R.fix(m, np.zeros(4, np.int32), 1)
    assert list(part) == [0, 0, 0, 0]
    assert st == dict(ncomp=2, nmerged=0, nmerged_tets=0, ncannot=1, counter=4)


def test_fix_foreign_target_and_missing_colour():
    """Marks outside the colour list are merge targets only; a colour with no
    tet is passed over.  Colour 4 = {1, 2} and {4}; {4} merges into tet 5
    (face 0 before face 3), mark 9, never processed: counter - 1."""
    m = chains(6)
    part, st = R.fix(m, np.array([4, 4, 9, 4, 9, 9], np.int32), [1, 4, 7])
    assert list(part) == [4, 4, 9, 9, 9, 9]
    assert st == dict(ncomp=4, nmerged=1, nmerged_tets=1, ncannot=0, counter=2)


# ---- the planted cases run the paths they are named for ------------------------------------

def test_planted_cases_exercise_their_paths():
    m, part, col, fpart, st = R.case("planted12")
    assert st["nmerged"] >= 10 and st["ncannot"] == 0
    before = R.components(m, part, 4)[1]
    assert before[0] > 1 and before[2] > 1 and before[3] == 2
    assert list(R.components(m, fpart, 4)[1]) == [1, 1, 1, 1]
    # the blob across the boundary of colours 1 and 2 went one way, whole
    blob = R.plant(m, part.copy(), [R.nearest(m, 0.5, 0.2, 0.667)], 0, 12)
    assert np.all(part[blob] == 0) and len(set(fpart[blob])) == 1
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) // 4
    around = nb[blob][nb[blob] > 0] - 1
    assert {1, 2} <= set(part[around])
    # equal sizes: the later piece of colour 3 lost
    three = np.nonzero(part == 3)[0]
    assert len(three) == 10 and list(fpart[three[:1]]) == [3] and (fpart == 3).sum() == 5
    assert fpart[three[0]] == 3 and fpart[three[-1]] != 3

    m, part, col, fpart, st = R.case("cascade6")
    assert R.components(m, part, 3)[1][2] == 2 and R.components(m, fpart, 3)[1][2] == 1
    assert st["nmerged"] == 1 and st["nmerged_tets"] == 216 and np.all(fpart[part == 2] == 2)

    assert R.case("unset_small_first")[4]["ncannot"] == 2 and R.case("unset_small_first")[4]["nmerged"] == 0
    st = R.case("unset_large_first")[4]
    assert st["ncannot"] == 1 and st["nmerged"] == 1

    m, part, col, fpart, st = R.case("interface6")
    assert st["nmerged"] > 0 and st["counter"] < m.ne
    foreign = ~np.isin(part, col)
    assert set(part[foreign]) >= {0, 2, 3, 5}
    assert np.array_equal(fpart[foreign], part[foreign])        # foreign tets are never listed
    for name in ("wave_bisect", "wave_random", *R.RANDOM_CASES):
        st = R.case(name)[4]
        assert st["nmerged"] > (50 if name != "wave_bisect" else 20), name


def test_counter_goes_down_for_unprocessed_targets_only():
    """3 slabs: a colour-0 fragment inside colour 2 is counted in colour 0's
    turn, taken off again (its target has not had its turn) and counted with
    colour 2; a colour-2 fragment inside colour 0 is counted once."""
    m = M.kuhn_cube(6)
    pick = lambda x, y, z: R.nearest(m, x, y, z)
    base = R.slabs(m, 3)
    p = base.copy()
    R.plant(m, p, [pick(0.5, 0.5, 0.9)], 0, 3)
    part, st = R.fix(m, p, 3)
    assert np.array_equal(part, base) and st["counter"] == m.ne and st["nmerged_tets"] == 3
    p = base.copy()
    R.plant(m, p, [pick(0.5, 0.5, 0.1)], 2, 3)
    part, st = R.fix(m, p, 3)
    assert np.array_equal(part, base) and st["counter"] == m.ne and st["nmerged_tets"] == 3
    # only colour 0 processed: the fragment taken off is not counted again
    p = base.copy()
    R.plant(m, p, [pick(0.5, 0.5, 0.9)], 0, 3)
    part, st = R.fix(m, p, [0])
    assert st["counter"] == (base == 0).sum()


def test_reversed_colour_order_differs():
    m, part, col, fpart, _ = R.case(R.RANDOM_CASES[0])
    rpart, _ = R.fix(m, part, np.arange(col)[::-1])
    assert not np.array_equal(rpart, fpart)


# ---- declarations ---------------------------------------------------------------------

def test_header_and_binding_declare_the_calls():
    hdr = open(os.path.join(ROOT, "include", "pmx_transfer.h")).read()
    for name in ("pmx_contiguity", "pmx_fix_contiguity"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in N.SIGNATURES
    assert "pmx_contig_stats" in hdr
    assert [f for f, _ in N.ContigStats._fields_] == ["ncomp", "nmerged", "nmerged_tets", "ncannot", "counter",
                                                      "rounds", "relabels", "replays", "replay_steps"]


def test_library_exports_the_calls():
    try:
        lib = N.load()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"the HIP library does not load on this machine: {e}")
    assert hasattr(lib, "pmx_contiguity") and hasattr(lib, "pmx_fix_contiguity")
