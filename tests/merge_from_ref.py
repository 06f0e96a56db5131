"""What pmx_merge_groups_from must return for groups that are not packed, from
the twin of the merge (merge_ref) and numpy alone (test infrastructure).

A group is the dict merge_ref takes: tetra_v ((ne+1, 4), row 0 unused; a row
with v[0] <= 0 is a deleted tet), xyz, sols, node_index1/2, face_index1/2, all
in the group's own numbering.  Packing is the stable compaction the library
documents: a point that no valid tet holds and a deleted tet are dropped, the
survivors keep their order."""
import numpy as np

import merge_ref as R

IDX = ("node_index1", "node_index2", "face_index1", "face_index2")


def _idx(grp, k):
    return np.ascontiguousarray(grp.get(k, np.zeros(0)), np.int32)


def pack_maps(grp):
    """(point_new (np+1,), tet_new (ne+1,)): the packed id of every own id, 0 for a dropped one."""
    tv = np.asarray(grp["tetra_v"], np.int32)
    npo = grp["xyz"].shape[0] - 1
    tvalid = np.zeros(tv.shape[0], bool)
    tvalid[1:] = tv[1:, 0] > 0
    used = np.zeros(npo + 1, bool)
    used[tv[tvalid].ravel()] = True
    pnew, tnew = np.zeros(npo + 1, np.int32), np.zeros(tv.shape[0], np.int32)
    pnew[used] = np.arange(1, used.sum() + 1)
    tnew[tvalid] = np.arange(1, tvalid.sum() + 1)
    return pnew, tnew


def pack_group(grp):
    """The packed group, and the own id of every packed point and tet
    (point_old (npk+1,), tet_old (nek+1,), entry 0 = 0)."""
    pnew, tnew = pack_maps(grp)
    pold = np.concatenate([[0], np.nonzero(pnew)[0]]).astype(np.int32)
    told = np.concatenate([[0], np.nonzero(tnew)[0]]).astype(np.int32)
    tv = np.asarray(grp["tetra_v"], np.int32)
    out = {"tetra_v": pnew[tv[told]], "xyz": np.ascontiguousarray(grp["xyz"][pold]),
           "sols": [np.ascontiguousarray(s[pold]) for s in grp["sols"]]}
    out["tetra_v"][0] = 0
    out["xyz"][0] = grp["xyz"][0]
    n1, f1 = _idx(grp, "node_index1"), _idx(grp, "face_index1")
    assert np.all(pnew[n1] > 0) and np.all(tnew[f1 // 12] > 0), "an entry names a dropped point or tet"
    out["node_index1"], out["node_index2"] = pnew[n1], _idx(grp, "node_index2")
    out["face_index1"], out["face_index2"] = (12 * tnew[f1 // 12] + f1 % 12).astype(np.int32), _idx(grp, "face_index2")
    return out, pold, told


def unpack_group(grp, point_holes, tet_holes):
    """A packed group renumbered with unused points at the own ids point_holes
    and deleted tets at the own ids tet_holes (the inverse of pack_group)."""
    npk, nek = grp["xyz"].shape[0] - 1, grp["tetra_v"].shape[0] - 1
    npo, neo = npk + len(point_holes), nek + len(tet_holes)
    pkeep = np.setdiff1d(np.arange(1, npo + 1), point_holes)
    tkeep = np.setdiff1d(np.arange(1, neo + 1), tet_holes)
    assert len(pkeep) == npk and len(tkeep) == nek
    pown = np.concatenate([[0], pkeep]).astype(np.int32)
    town = np.concatenate([[0], tkeep]).astype(np.int32)
    xyz = np.full((npo + 1, 3), 0.5)
    xyz[pown] = grp["xyz"]
    sols = []
    for s in grp["sols"]:
        a = np.full((npo + 1, s.shape[1]), -5.0)
        a[pown] = s
        sols.append(a)
    tv = np.zeros((neo + 1, 4), np.int32)
    tv[tkeep] = pown[np.asarray(grp["tetra_v"], np.int32)[1:]]
    f1 = _idx(grp, "face_index1")
    return {"tetra_v": tv, "xyz": xyz, "sols": sols,
            "node_index1": pown[_idx(grp, "node_index1")], "node_index2": _idx(grp, "node_index2"),
            "face_index1": (12 * town[f1 // 12] + f1 % 12).astype(np.int32), "face_index2": _idx(grp, "face_index2")}


def expected(groups, comm=None):
    """The twin's merge of the stably packed groups with tet_old, point_old and
    the maps composed back into the groups' own numbering."""
    packs = [pack_group(g) for g in groups]
    ref = R.merge([p[0] for p in packs], comm)
    pold, told = ref["point_old"].copy(), ref["tet_old"].copy()
    maps = []
    for g, (_, po, to) in enumerate(packs):
        at = ref["point_group"] == g
        pold[at] = po[ref["point_old"][at]]
        at = ref["tet_group"] == g
        told[at] = to[ref["tet_old"][at]]
        pn = np.zeros(groups[g]["xyz"].shape[0] - 1, np.int32)
        tn = np.zeros(groups[g]["tetra_v"].shape[0] - 1, np.int32)
        pn[po[1:] - 1] = ref["maps"][g][0]
        tn[to[1:] - 1] = ref["maps"][g][1]
        maps.append((pn, tn))
    return dict(ref, point_old=pold, tet_old=told, maps=maps)
