"""pmx_merge_groups_from without a GPU: the symbol and its declaration, the C
driver against the header, and the numpy helper the GPU tests take their
expectation for unpacked groups from (tests/merge_from_ref.py)."""
import os
import re
import subprocess

import numpy as np

import merge_from_ref as U
import merge_ref as R
import split_ref as S
from parmmg_amd import _native as N
from parmmg_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_exported_and_declared():
    assert "pmx_merge_groups_from" in N.SIGNATURES
    with open(os.path.join(ROOT, "include", "pmx_transfer.h"), encoding="utf-8") as fh:
        hdr = fh.read()
    assert re.search(r"^int pmx_merge_groups_from\(pmx_ctx \*ctx, int32_t ngrp, const pmx_merge_source \*", hdr, re.M)
    assert re.search(r"typedef struct \{ pmx_ctx \*held; pmx_merge_group g; \} pmx_merge_source;", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T pmx_merge_groups_from$", out, re.M)
    lib = N.load()
    assert lib.pmx_merge_groups_from.argtypes[2]._type_ is N.MergeSource
    # the struct the binding passes is the header's: a pointer, then the group
    assert [f[0] for f in N.MergeSource._fields_] == ["held", "g"]


def test_demo_compiles_against_the_header(tmp_path):
    src = os.path.join(ROOT, "tests", "c", "merge_from_demo.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                    "-c", src, "-o", str(tmp_path / "merge_from_demo.o")], check=True)


def groups_of(n, nparts):
    m = M.kuhn_cube(n)
    sp, comm = R.split_case(m, S.slabs(m, nparts), nparts, R.sols_of(m))
    return sp["groups"], comm


def same_group(a, b):
    assert np.array_equal(a["tetra_v"], b["tetra_v"]) and a["xyz"][1:].tobytes() == b["xyz"][1:].tobytes()
    for x, y in zip(a["sols"], b["sols"]):
        assert x[1:].tobytes() == y[1:].tobytes()
    for k in U.IDX:
        assert np.array_equal(a[k], b[k]), k


def test_packing_a_packed_group_is_the_identity():
    """... so that the expectation for unpacked groups reduces to the twin's
    merge itself for packed ones."""
    groups, comm = groups_of(3, 3)
    for g in groups:
        packed, pold, told = U.pack_group(g)
        same_group(packed, g)
        assert np.array_equal(pold, np.arange(len(pold))) and np.array_equal(told, np.arange(len(told)))
    ref, exp = R.merge(groups, comm), U.expected(groups, comm)
    for k in R.INT_KEYS:
        assert np.array_equal(ref[k], exp[k]), k
    for (a, b), (c, d) in zip(ref["maps"], exp["maps"]):
        assert np.array_equal(a, c) and np.array_equal(b, d)


def test_unpack_then_pack_returns_the_group():
    groups, comm = groups_of(4, 2)
    ref = R.merge(groups, comm)
    holes = []
    for g in groups:
        npk, nek = g["xyz"].shape[0] - 1, g["tetra_v"].shape[0] - 1
        holes.append((np.array([1, 7, 8, npk + 4]), np.array([1, 2, 30, nek + 4])))
    own = [U.unpack_group(g, ph, th) for g, (ph, th) in zip(groups, holes)]
    for g, o, (ph, th) in zip(groups, own, holes):
        packed, pold, told = U.pack_group(o)
        same_group(packed, g)
        pn, tn = U.pack_maps(o)
        assert np.all(pn[ph] == 0) and np.all(tn[th] == 0) and (pn > 0).sum() == g["xyz"].shape[0] - 1
        assert np.all(o["tetra_v"][th, 0] <= 0)
    exp = U.expected(own, comm)
    # the merged mesh is the packed groups'; the old ids and the maps are in the own numbering
    for k in ("tetra_v", "tet_group", "point_group", "node_index1", "node_index2", "face_index1", "face_index2"):
        assert np.array_equal(exp[k], ref[k]), k
    for g, o in enumerate(own):
        _, pold, told = U.pack_group(o)
        at = ref["tet_group"] == g
        assert np.array_equal(exp["tet_old"][at], told[ref["tet_old"][at]])
        pn, tn = exp["maps"][g]
        assert len(pn) == o["xyz"].shape[0] - 1 and len(tn) == o["tetra_v"].shape[0] - 1
        assert np.array_equal(pn[pold[1:] - 1], ref["maps"][g][0]) and np.array_equal(tn[told[1:] - 1], ref["maps"][g][1])
        assert np.all(pn[holes[g][0] - 1] == 0) and np.all(tn[holes[g][1] - 1] == 0)
        # a merged tet's old id names the tet it came from: same vertices through the point map
        k = np.nonzero(at)[0]
        assert np.array_equal(pn[o["tetra_v"][exp["tet_old"][k]] - 1], exp["tetra_v"][k + 1])
