"""integration/pmmg_pmx.c with more solution fields than the fused step
carries: tests/c/manyfields_demo.c calls the binding's
PMMG_copyMetricsAndFields_point and PMMG_interpMetricsAndFields (exact
reference signatures, tests/c/pmmg_stub/parmmg.h) on one group with the metric
and mesh->nsols = 12 fields.  The fields against the oracle and, bit for bit,
against the library's own step + interp_more on the same inputs."""
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import bits_equal, compare_volume
from oracle import oracle as O
from parmmg_amd import mesh as M
from test_gpu_many_fields import spd_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "integration", "pmmg_pmx.c"), os.path.join(ROOT, "tests", "c", "manyfields_demo.c")]
BIN = os.path.join(ROOT, "tests", "c", "_build", "manyfields_demo")
NFLD = 12
SENT = -7.0


def build_manyfields_demo() -> str:
    """The gcc line of test_adapter.build_adapter_demo."""
    from parmmg_amd import build
    lib = build.build_transfer()
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    deps = SRC + [os.path.join(ROOT, "include", "pmx_transfer.h"),
                  os.path.join(ROOT, "tests", "c", "pmmg_stub", "parmmg.h"), lib]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1",
                        "-I", os.path.join(ROOT, "tests", "c", "pmmg_stub"), "-I", os.path.join(ROOT, "include"),
                        *SRC, "-L", os.path.dirname(lib), "-lpmx_transfer",
                        f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", BIN], check=True)
    return BIN


def test_manyfields_demo_compiles_as_c():
    """The binding with its view arrays sized by mesh->nsols still compiles as
    C99 with -Wall -Wextra -Werror (no GPU needed)."""
    assert os.path.exists(build_manyfields_demo())


def write_case(d, n=6, n2=7):
    """test_adapter.write_case's meshes (a background Kuhn cube, a new mesh
    from another one, a few frozen vertices kept in place), with 12 fields of
    sizes cycling 1, 3, 6."""
    old = M.kuhn_cube(n, seed=3)
    new = M.kuhn_cube(n2, seed=4)
    otag = np.zeros(old.np + 1, np.uint16)
    onb = np.any((old.xyz[1:] == 0.0) | (old.xyz[1:] == 1.0), axis=1)
    otag[1:][onb] = M.TAG_BDY
    req = np.arange(1, min(old.np, new.np) + 1, 13)
    otag[req] |= M.TAG_REQ
    ntag = np.zeros(new.np + 1, np.uint16)
    nnb = np.any((new.xyz[1:] == 0.0) | (new.xyz[1:] == 1.0), axis=1)
    ntag[1:][nnb] = M.TAG_BDY
    ntag[req] = otag[req]
    nxyz = new.xyz.copy()
    nxyz[req] = old.xyz[req]
    rng = np.random.default_rng(31)
    omet = M.on_vertices(old, M.iso_metric)
    sizes = [(1, 3, 6)[k % 3] for k in range(NFLD)]
    oflds = [spd_field(old.np + 1, rng) if sz == 6 else rng.normal(size=(old.np + 1, sz)) for sz in sizes]
    files = dict(old_xyz=old.xyz, old_tet=old.tet, old_tag=otag, old_met=omet, new_xyz=nxyz, new_tet=new.tet,
                 new_tag=ntag)
    for j, a in enumerate(oflds):
        files[f"old_fld_{j}"] = a
    for k, a in files.items():
        np.ascontiguousarray(a).tofile(os.path.join(d, k + ".bin"))
    with open(os.path.join(d, "sizes.txt"), "w") as fh:
        fh.write(f"{old.np} {old.ne} {new.np} {new.ne} {omet.shape[1]} {NFLD}\n")
        fh.write(" ".join(str(s) for s in sizes) + "\n")
    return old, new, otag, ntag, nxyz, omet, oflds, req


@pytest.mark.gpu
def test_binding_twelve_fields(tmp_path):
    d = str(tmp_path)
    old, new, otag, ntag, nxyz, omet, oflds, req = write_case(d)
    r = subprocess.run([build_manyfields_demo(), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    calls = {c["call"]: c["ret"] for c in (json.loads(s) for s in r.stdout.splitlines() if s.startswith("{"))}
    assert calls == {"copy": 1, "interp": 1}, calls
    olds = [omet] + oflds
    got = [np.fromfile(os.path.join(d, "out_met.bin")).reshape(new.np + 1, 1)]
    got += [np.fromfile(os.path.join(d, f"out_fld_{j}.bin")).reshape(new.np + 1, a.shape[1])
            for j, a in enumerate(oflds)]
    # frozen points: the old values (the copy), untouched by the interpolation
    for g, o in zip(got, olds):
        assert np.array_equal(g[req], o[req])
    x, t = nxyz[1:], ntag[1:]
    live = (t & M.TAG_REQ) == 0
    # the library's own step (metric + 7 fields) + interp_more (the other 5)
    from parmmg_amd.transfer import Transfer
    tr = Transfer(0)
    try:
        tr.upload_background(old, olds[:8], 0)
        tr.upload_points(x, t, tets_mmg=new.tet)
        tr.run()
        res = tr.download(init=[np.full((len(x), a.shape[1]), SENT) for a in olds[:8]])
        more = tr.interp_more(olds[8:], init=[np.full((len(x), a.shape[1]), SENT) for a in olds[8:]])
    finally:
        tr.close()
    dev = res.sols + more
    for k, (g, w) in enumerate(zip(got, dev)):
        assert not np.any(w[live] == SENT), f"solution {k} has unwritten live rows"
        assert bits_equal(g[1:][live], w[live]).all(), f"solution {k} differs from step + interp_more"
    # and the oracle, all 13 solutions in one call
    o = O.Oracle(old)
    outs, elem, st, *_ = o.interp(x, t, olds, imet=0)
    c = compare_volume(o, x, t, ([g[1:] for g in got], res.elem, res.status), (outs, elem, st), olds)
    assert c["nvol"] > 100 and c["same"] >= c["nvol"] - max(3, c["nvol"] // 1000)
