"""The CPU twin of the interface displacement (tests/c/moveifc_ref.c) against
independent numpy / Python: begin as a two-pass minimum, the invariants of a
layer, and the parallel formulation of DESIGN.md section 4 ("Interface
displacement") restated in Python (moveifc_ref.model_layer), which must give the twin's bytes on every layer
its block predicate lets through -- and the predicate must hold exactly when
the twin did not block.  No GPU."""
import numpy as np
import pytest

import moveifc_ref as F

CUBE_CASES = [c for c in F.CASES if not c.startswith(("wave", "cone"))]


def weights_of(t, color):
    return t.weight(np.asarray(color)).astype(np.int64)


ball, model_layer = F.ball, F.model_layer


@pytest.mark.parametrize("name", ["revquad", "ties", "frag_6_counts", "wave_bisect", "ranks3", "corner"])
def test_begin_is_a_two_pass_minimum(name):
    m, tg, mp, node, begin, layers, t = F.run(name)
    mark = (t.nprocs * tg + t.myrank).astype(np.int64)
    assert np.array_equal(begin["mark"], mark)
    pts = m.tet[1:].ravel().astype(np.int64)             # slot 4 k + j at index 4 (k - 1) + j
    slots = np.arange(4, 4 * m.ne + 4, dtype=np.int64)
    wslot = weights_of(t, np.repeat(mark, 4))
    first = np.full(m.np + 1, 1 << 40)
    wbest = np.full(m.np + 1, 1 << 40)
    np.minimum.at(first, pts, slots)
    np.minimum.at(wbest, pts, wslot)
    sbest = np.full(m.np + 1, 1 << 40)
    hit = wslot == wbest[pts]
    np.minimum.at(sbest, pts[hit], slots[hit])
    used = first[1:] < (1 << 40)
    assert used.all()
    assert np.array_equal(begin["s"], sbest[1:])
    assert np.array_equal(begin["tmp"], mark[sbest[1:] // 4 - 1])
    front = wbest[1:] < weights_of(t, mark[first[1:] // 4 - 1])
    assert np.array_equal(begin["front"], front.astype(np.int32))
    assert begin["nfront"] == front.sum()
    own = mp["mapgrp"][mp["displsgrp"][t.myrank]:mp["displsgrp"][t.myrank + 1]]
    assert np.array_equal(begin["negrp"], own)
    assert np.array_equal(begin["nemin"], np.minimum(6, own // 2 + 1))


@pytest.mark.parametrize("name", ["empty_slabs", "equal_slabs"])
def test_lighter_groups_first_give_an_empty_front(name):
    m, tg, mp, node, begin, layers, t = F.run(name)
    assert begin["nfront"] == 0
    for ok, st, snap in layers:
        assert ok and st["front"] == 0 and st["recolor"] == 0
        assert all(np.array_equal(snap[k], begin[k]) for k in ("mark", "tmp", "s", "front", "negrp"))


@pytest.mark.parametrize("name", CUBE_CASES)
def test_layer_invariants(name):
    m, tg, mp, node, begin, layers, t = F.run(name)
    for li, (ok, st, post) in enumerate(layers):
        assert ok
        pre = t.pres[li]                                 # the layer's start, after its exchange
        if node is not None:
            assert pre["front"][node[0] - 1].all()      # every listed point is front
        # weights only ever decrease
        assert (weights_of(t, post["mark"]) <= weights_of(t, pre["mark"])).all()
        # recoloured tets lie in the balls of the layer's front points
        fronts = np.nonzero(pre["front"] & (pre["s"] >= 0))[0] + 1
        inball = np.zeros(m.ne + 1, bool)
        for p in fronts:
            inball[[sl // 4 for sl in ball(m, int(pre["s"][p - 1]))]] = True
        changed = np.nonzero(post["mark"] != pre["mark"])[0] + 1
        assert inball[changed].all()
        assert st["front"] == len(fronts)
        # negrp: never below nemin, lost at least the tets that left each local
        # group.  Snapshots cannot give the exact count: a tet recoloured twice
        # in a layer shows one change, and a blocked layer has no independent
        # model; the exact per-group count is asserted on every clean layer in
        # test_parallel_formulation_equals_the_twin (the model's D).
        loss = pre["negrp"] - post["negrp"]
        local = pre["mark"] % t.nprocs == t.myrank
        left = np.bincount(pre["mark"][local & (post["mark"] != pre["mark"])] // t.nprocs, minlength=t.nold)
        assert (loss >= left).all() and (post["negrp"] >= np.minimum(begin["nemin"], begin["negrp"])).all()
        assert loss.sum() <= st["recolor"]
        assert st["next"] == post["front"].sum()


@pytest.mark.parametrize("name", CUBE_CASES)
def test_parallel_formulation_equals_the_twin(name):
    """Cases 2-4 run clean (asserted below), every other case checks the
    predicate and compares the layers it lets through; the three-rank cases
    run with the exchange applied between the layers (t.pres)."""
    m, tg, mp, node, begin, layers, t = F.run(name)
    for li, (ok, st, post) in enumerate(layers):
        pre = t.pres[li]
        model, D, nrec, ntouched, balls, nforeign = model_layer(m, t, pre)
        clean = bool((pre["negrp"] - D >= pre["nemin"]).all())
        assert clean == (st["blocks"] == 0), (name, li)
        if not clean:
            continue
        for k in ("mark", "tmp", "s", "front", "negrp"):
            assert np.array_equal(model[k], post[k]), (name, li, k)
        # negrp equals start minus the changes from local colours, per group
        assert np.array_equal(pre["negrp"] - post["negrp"], D) and D.sum() + nforeign == nrec
        assert (nrec, ntouched) == (st["recolor"], st["touched"])
        assert st["maxball"] == max([len(b) for b in balls.values()], default=0)


def test_foreign_colours_on_the_parallel_path():
    """ranks3_big never blocks, tets are recoloured from foreign colours, and
    those recolourings are not counted in negrp."""
    m, tg, mp, node, begin, layers, t = F.run("ranks3_big")
    from_foreign = 0
    for li, (ok, st, post) in enumerate(layers):
        pre = t.pres[li]
        assert ok and st["blocked"] == 0
        _, D, nrec, _, _, nforeign = model_layer(m, t, pre)
        changed = post["mark"] != pre["mark"]
        from_foreign += int((changed & (pre["mark"] % t.nprocs != t.myrank)).sum())
        assert np.array_equal(pre["negrp"] - post["negrp"], D) and D.sum() == st["recolor"] - nforeign
        if st["recolor"] == changed.sum():               # no tet changed twice: the snapshots count exactly
            local = changed & (pre["mark"] % t.nprocs == t.myrank)
            assert np.array_equal(D, np.bincount(pre["mark"][local] // t.nprocs, minlength=t.nold))
    assert from_foreign > 0
    assert (layers[-1][2]["mark"] % t.nprocs != t.myrank).any()


def test_the_cases_meet_their_conditions():
    run = lambda n: [(st["blocked"], st) for ok, st, _ in F.run(n)[5]]
    assert [b for b, _ in run("revquad")] == [0, 0, 0]
    assert [st["front"] for _, st in run("revquad")] == [49, 97, 97]
    assert [b for b, _ in run("octants")] == [0, 0, 1]
    assert [b for b, _ in run("ties")] == [0, 0, 0, 0]
    ties = run("ties")
    changed = (F.run("ties")[5][0][2]["mark"] != F.run("ties")[4]["mark"]).sum()
    assert ties[0][1]["recolor"] > changed               # tets recoloured twice in one layer
    assert ties[3][1]["next"] == 0                       # the front dies out
    assert all(b == 0 for n in ("frag_4_big", "frag_6_big") for b, _ in run(n))
    assert [b for b, _ in run("frag_6_counts")][:2] == [1, 1]
    assert [b for b, _ in run("revslabs")] == [0, 1]
    m, tg, mp, node, begin, layers, t = F.run("tiny")
    assert ((begin["negrp"] == begin["nemin"]) & (begin["negrp"] <= 2)).sum() == 2
    assert any(st["blocked"] for _, st, _ in layers)


def test_three_ranks_take_foreign_colours():
    m, tg, mp, node, begin, layers, t = F.run("ranks3")
    final = layers[-1][2]
    foreign = final["mark"] % 3 != 1
    assert foreign.any()                                 # tets took foreign colours
    assert set(np.unique(final["mark"][foreign])) <= {0, 2, 5}
    ok, part, ngrp = t.part(2)
    assert not ok                                        # MMG_TARGET refuses a foreign colour
    ok, part, ngrp = t.part(1)
    assert ok and np.bincount(part, minlength=ngrp).sum() == m.ne
    assert (np.bincount(part, minlength=ngrp) > 0).all() and part.max() == ngrp - 1
    # the ranks are visited from myrank round: an own colour comes first
    own_first = part[np.nonzero(final["mark"] % 3 == 1)[0]].min()
    assert own_first == 0
    # a clean single-rank run: MMG_TARGET gives the old groups back
    m2, tg2, mp2, _, _, lay2, t2 = F.run("revquad")
    ok, part2, n2 = t2.part(2)
    assert ok and n2 == 4 and np.array_equal(part2, lay2[-1][2]["mark"])
    assert np.bincount(part2, minlength=4).sum() == m2.ne


def test_a_ball_that_is_not_face_connected_is_walked_on_one_side():
    m, tg, mp, node, begin, layers, t = F.run("corner")
    _, ne_a, corner = F.two_cubes_corner(2)
    assert begin["front"][corner - 1] == 1
    assert begin["s"][corner - 1] // 4 > ne_a            # its slot lies in the second cube
    final = layers[-1][2]
    at_corner = np.nonzero((m.tet[1:ne_a + 1] == corner).any(1))[0]
    assert len(at_corner) and (weights_of(t, begin["mark"][at_corner]) > weights_of(t, begin["tmp"][corner - 1])).all()
    assert np.array_equal(final["mark"][at_corner], begin["mark"][at_corner])


def test_ball_overflow():
    m, tg, mp, node, begin, layers, t = F.run("cone_71")
    assert layers[0][0] and layers[0][1]["maxball"] == 2 * 71 * 71 == F.LMAX - 158
    m, tg, mp, node, begin, layers, t = F.run("cone_72")
    _, apex = F.cone(72)
    ok, st, _ = layers[0]
    assert not ok and st["overflow_ip"] == apex and m.ne == 10368 > F.LMAX - 2
