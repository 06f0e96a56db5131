"""The oracle's point location against a brute-force long-double definition.

tests/reference_locate.py states, from the mesh alone and without any walk,
what a correct location must satisfy: which tets / trias hold a point, which
is the closest when none does, and the wedge / cone predicates.  Here the
oracle -- the checker of every GPU test -- is run through it on the inputs of
tests/locate_cases.py (every branch occurs: found, exhaustive, not found,
ties, deleted tets, shuffled numbering; inside, border edge / vertex, wedge,
cone, exhaustive, not found on the surface), in reference semantics and, for
the surface, in the device's (fresh point flags at every query).

Teeth: every mutation of the oracle's answer listed in test_*_mutations makes
the check fail on the mutated (decidable) points.
"""
import numpy as np
import pytest

import locate_cases as LC
import reference_hp as R
import reference_locate as RL
from oracle import oracle as O
from parmmg_amd import mesh as M

LD = np.longdouble


def oracle_volume(name):
    m, x = LC.volume_case(name)
    _, elem, st, *_ = O.Oracle(m).interp(x, np.zeros(len(x), np.uint16), [], imet=-1)
    return m, x, elem, st, LC.volume_reference(name)


def oracle_surface(name, fresh=True):
    m, x = LC.surface_case(name)
    _, elem, st, _, e, v = O.Oracle(m).interp(x, np.full(len(x), M.TAG_BDY, np.uint16), [], imet=-1, fresh=fresh)
    return m, x, elem, st, e, v, LC.surface_reference(name)


def bad_points(rep):
    return sorted({i for i, _ in rep["violations"]})


# ---- the definitions themselves ---------------------------------------------------

def test_lambdas_are_barycentrics():
    """The determinant ratios sum to 1, reproduce the point, and agree with
    reference_hp's solve (another formula) far below the thresholds' 1e-9."""
    m, x = LC.volume_case("ties")
    rng = np.random.default_rng(1)
    ks = rng.integers(1, m.ne + 1, len(x))
    P = m.xyz[m.tet[ks]]
    lam, vol = RL.tet_lambdas(P, x)
    assert np.all(vol > 0) and np.abs(lam.sum(1) - 1).max() < 1e-17
    assert np.abs(np.einsum("nk,nkd->nd", lam, np.asarray(P, LD)) - x).max() < 1e-17
    assert np.abs(lam - R.bary_tet(P, x)).max() < 1e-15
    m, x = LC.surface_case("cube6")
    ks = rng.integers(1, m.nt + 1, len(x))
    P = m.xyz[m.tria[ks]]
    lam, h = RL.tria_lambdas(P, x)
    assert np.abs(lam.sum(1) - 1).max() < 1e-17
    assert np.abs(lam - R.bary_tria(P, x)).max() < 1e-15
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    q = np.einsum("nk,nkd->nd", lam, np.asarray(P, LD)) + h[:, None] * nrm
    assert np.abs(q - x).max() < 1e-15


# ---- the oracle against the definition --------------------------------------------

@pytest.mark.parametrize("name", LC.VOLUME)
def test_oracle_volume(name):
    m, x, elem, st, ref = oracle_volume(name)
    rep = RL.check_volume(m, x, elem, st, False, ref)
    print(name, RL.summary(rep))
    assert not rep["violations"], rep["violations"][:5]
    assert rep["undecidable"] == 0
    LC.assert_min_counts(rep, LC.VOLUME_MIN[name], name)
    assert np.array_equal(st != 0, ref["nC"] > 0)
    if name == "ties":
        # the reference's walk does not return min C: the canonical rule is the device's own
        assert 50 <= (elem != ref["minC"]).sum() <= 150
    if name == "deleted":
        dead = LC.holes(name)
        assert len(dead) > 50 and not ref["inC"][:, dead].any() and not np.isin(elem, dead).any()
        planted = np.arange(600, len(x))                  # the points inside deleted tets
        assert len(planted) >= 15 and np.all(ref["nC"][planted] == 0) and np.all(st[planted] == 0)
    if name == "shuffled":
        base = LC.volume_reference("lshape")                # the same 600 points, then 80 tie points
        assert np.array_equal(ref["nC"][:600], base["nC"])
        assert (ref["minC"][:600] != base["minC"])[base["nC"] > 0].mean() > 0.9
        assert (ref["closest"][:600] != base["closest"]).mean() > 0.9
        assert (elem != ref["minC"])[600:].sum() >= 10


@pytest.mark.parametrize("fresh", [False, True], ids=["reference", "fresh"])
@pytest.mark.parametrize("name", LC.SURFACE)
def test_oracle_surface(name, fresh):
    m, x, elem, st, e, v, ref = oracle_surface(name, fresh)
    rep = RL.check_surface(m, x, elem, st, e, v, ref)
    print(name, RL.summary(rep))
    assert not rep["violations"], rep["violations"][:5]
    assert rep["undecidable"] == 0 and not rep["skipped"]
    LC.assert_min_counts(rep, LC.SURFACE_MIN[name], name)
    LC.assert_min_counts(rep, LC.SURFACE_MIN_ORACLE.get(name, {}), name)
    assert np.all(st[ref["nT"] > 0] != 0)
    if name.endswith("_h002"):
        # the populations move with hausd
        big = RL.check_surface(*oracle_surface(name[:-5], fresh))
        assert rep["not_found"] >= big["not_found"] + 250
        assert rep["wedge"] + rep["cone"] <= (big["wedge"] + big["cone"]) // 10


def test_cone_flag_skip_is_the_reference():
    """One point of this input is accepted by a cone although a neighbour of
    the vertex lies on the point's side (the full predicate fails): the
    reference flags a neighbour before testing it and skips flagged ones
    (src/locate_pmmg.c:248-249), so the second cone test at that vertex no
    longer sees the neighbour that rejected the first.  The checker reports it
    as cone_skip, not as a violation; everything else holds."""
    for fresh in (False, True):
        m, x, elem, st, e, v, ref = oracle_surface("wave_skip", fresh)
        rep = RL.check_surface(m, x, elem, st, e, v, ref)
        assert not rep["violations"] and rep["undecidable"] == 0
        assert rep["cone_skip"] == 1 and len(rep["skipped"]) == 1
        i = rep["skipped"][0]
        ok, und, near = RL._cone(m, int(elem[i]), int(v[i]), np.asarray(x[i], LD), ref["hausd"], ref["fan"])
        assert near and not ok and not und and ref["nT"][i] == 0


# ---- mutations --------------------------------------------------------------------

def test_volume_mutations():
    m, x, elem, st, ref = oracle_volume("lshape")
    found, lost = np.nonzero(st != 0)[0], np.nonzero(st == 0)[0]
    # a face neighbour that does not hold the point
    adj = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) // 4
    mut, hit = elem.copy(), []
    for i in found:
        nb = [k for k in adj[elem[i] - 1] if k > 0 and not ref["inC"][i, k]]
        if nb:
            mut[i] = nb[0]
            hit.append(i)
    assert len(hit) > 200
    assert bad_points(RL.check_volume(m, x, mut, st, False, ref)) == hit
    # a not-found point given its second-closest tet
    mut = elem.copy()
    mut[lost] = ref["second"][lost]
    assert bad_points(RL.check_volume(m, x, mut, st, False, ref)) == lost.tolist()
    # status 1 -> 0 and 0 -> 1
    assert bad_points(RL.check_volume(m, x, elem, np.where(st != 0, 0, st), False, ref)) == found.tolist()
    assert bad_points(RL.check_volume(m, x, elem, np.where(st == 0, 1, st), False, ref)) == lost.tolist()
    assert bad_points(RL.check_volume(m, x, elem, np.where(st == 0, -1, st), False, ref)) == lost.tolist()
    # a tie answered with a non-minimal member: only the canonical check objects
    m, x, elem, st, ref = oracle_volume("ties")
    tied = np.nonzero(ref["nC"] > 1)[0]
    mut = elem.copy()
    mut[tied] = m.ne - np.argmax(ref["inC"][tied, ::-1], axis=1)       # max C
    assert np.all(ref["inC"][tied, mut[tied]]) and np.all(mut[tied] > ref["minC"][tied])
    assert not RL.check_volume(m, x, mut, st, False, ref)["violations"]
    assert bad_points(RL.check_volume(m, x, mut, st, True, ref)) == tied.tolist()
    canon = np.where(ref["nC"] > 0, ref["minC"], elem)
    assert not RL.check_volume(m, x, canon, st, True, ref)["violations"]
    # a deleted tet returned
    m, x, elem, st, ref = oracle_volume("deleted")
    dead = LC.holes("deleted")
    mut = elem.copy()
    mut[::5] = dead[np.arange(len(mut[::5])) % len(dead)]
    assert bad_points(RL.check_volume(m, x, mut, st, False, ref)) == list(range(0, len(x), 5))


def test_surface_mutations():
    m, x, elem, st, e, v, ref = oracle_surface("wave")
    base = RL.check_surface(m, x, elem, st, e, v, ref)
    assert not base["violations"]
    lost = np.nonzero(st == 0)[0]
    # a not-found point given the tria with the second-nearest centroid
    mut = elem.copy()
    mut[lost] = ref["second"][lost]
    assert bad_points(RL.check_surface(m, x, mut, st, e, v, ref)) == lost.tolist()
    # status 1 / -1 -> 0 and 0 -> 1: nothing found reported as not found, and the reverse
    held = np.nonzero(ref["nT"] > 0)[0]
    got = bad_points(RL.check_surface(m, x, elem, np.zeros_like(st), e, v, ref))
    assert set(held) <= set(got) and len(held) > 800
    one = np.where(st == 0, 1, st)
    assert bad_points(RL.check_surface(m, x, elem, one, e, v, ref)) == lost.tolist()
    # edge l -> (l + 1) % 3, on border edges and wedges alike
    on_edge = np.nonzero(e != -1)[0]
    assert len(on_edge) >= 150
    assert bad_points(RL.check_surface(m, x, elem, st, np.where(e != -1, (e + 1) % 3, e), v, ref)) == on_edge.tolist()
    # a border edge / vertex not reported
    on_vert = np.nonzero(v != -1)[0]
    plain = np.full_like(e, -1)
    got = bad_points(RL.check_surface(m, x, elem, st, plain, plain, ref))
    assert got == sorted(on_edge.tolist() + on_vert.tolist())
    # vertex moved to another corner, own vertices and cones alike
    assert len(on_vert) >= 100
    for d in (1, 2):
        got = bad_points(RL.check_surface(m, x, elem, st, e, np.where(v != -1, (v + d) % 3, v), ref))
        assert got == on_vert.tolist()
    # the checker at 2 x hausd against answers computed at hausd: missed trias
    ref2 = RL.surface_ref(m, x, hausd=2 * m.hausd)
    rep = RL.check_surface(m, x, elem, st, e, v, ref2)
    missed = [i for i, why in rep["violations"] if why.startswith("status 0 but")]
    assert len(missed) >= 200 and set(missed) == set(np.nonzero((st == 0) & (ref2["nT"] > 0))[0])


def test_wedge_and_cone_mutations():
    m, x, elem, st, e, v, ref = oracle_surface("ridge")
    rep = RL.check_surface(m, x, elem, st, e, v, ref)
    assert not rep["violations"] and rep["wedge"] >= 200 and rep["cone"] >= 40
    # a wedge point moved to 1.5 hausd from its edge (same alpha, same answers)
    wedge = np.nonzero(e != -1)[0]
    y = x.copy()
    for i in wedge:
        c0, c1 = m.xyz[m.tria[elem[i], (e[i] + 1) % 3]], m.xyz[m.tria[elem[i], (e[i] + 2) % 3]]
        a = c1 - c0
        foot = c0 + (a @ (x[i] - c0)) / (a @ a) * a
        r = x[i] - foot
        y[i] = foot + r * (1.5 * m.hausd / np.linalg.norm(r))
    assert bad_points(RL.check_surface(m, y, elem, st, e, v, RL.surface_ref(m, y))) == wedge.tolist()
    # a cone point moved 1.5 hausd away from its vertex, and one moved to the far side of a neighbour
    cone = np.nonzero(v != -1)[0]
    y, z = x.copy(), x.copy()
    for i in cone:
        tri = m.tria[elem[i]]
        c0 = m.xyz[tri[v[i]]]
        r = x[i] - c0
        y[i] = c0 + r * (1.5 * m.hausd / np.linalg.norm(r))
        z[i] = c0 + 0.3 * m.hausd * (m.xyz[tri[(v[i] + 1) % 3]] - c0) / np.linalg.norm(m.xyz[tri[(v[i] + 1) % 3]] - c0)
    assert bad_points(RL.check_surface(m, y, elem, st, e, v, RL.surface_ref(m, y))) == cone.tolist()
    rz = RL.check_surface(m, z, elem, st, e, v, RL.surface_ref(m, z))
    assert rz["skipped"] == cone.tolist() and rz["cone"] == 0      # never counted as cone answers
