"""bench.py's command line: a plain run times the steps and nothing else,
--full adds the other legs, --dump-outputs writes the last step's fields.

CPU: the dump's row sample (fixed, seeded, within the size cap) on stand-in
contexts.  GPU: one plain and one --full run of the smallest configuration
(C1) in child processes, their result lines and the dumped arrays against the
same case run in this process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT
from parmmg_amd.transfer import Result

FULL_ONLY = ("cpu_baseline", "locate", "resident_background_ms_per_step", "sequential_surface",
             "pcie_inclusive")
HEADLINE = {"metric": "new vertices located+interpolated/sec", "unit": "vertices/s",
            "higher_is_better": True, "dtype": "f64"}


class _Ctx:
    """What dump_outputs reads of a Transfer: npts, sizes, download()."""

    def __init__(self, n, sizes):
        self.npts, self.sizes = n, sizes
        self.sols = [np.arange(n * s, dtype=np.float64).reshape(n, s) + 0.5 * i for i, s in enumerate(sizes)]

    def download(self, sols_only=False):
        assert sols_only
        return Result(self.sols, None, None, None)


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_output_when_it_fits(tmp_path):
    c = _Ctx(1000, [1, 3])
    info = bench.dump_outputs([c], str(tmp_path), 0, 1)
    a = _load(tmp_path)
    assert sorted(a) == ["g0_rows.npy", "g0_sol0.npy", "g0_sol1.npy"] == sorted(info["files"])
    assert not info["sampled"] and all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["g0_rows.npy"], np.arange(1000))
    assert np.array_equal(a["g0_sol0.npy"], c.sols[0]) and np.array_equal(a["g0_sol1.npy"], c.sols[1])


def test_dump_sample_is_fixed_and_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 16)
    cs = [_Ctx(5000, [1, 1, 3]), _Ctx(4001, [1, 1, 3])]
    info = bench.dump_outputs(cs, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(cs, str(tmp_path / "b"), 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert info["sampled"] and len(a) == 8
    assert sum(v.nbytes for v in a.values()) <= 1 << 16
    assert all(v.dtype == np.float64 for v in a.values())
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    for g, c in enumerate(cs):
        rows = a[f"g{g}_rows.npy"].astype(np.int64)
        assert len(rows) == info["rows_per_group"] > 100
        assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < c.npts
        for i in range(3):
            assert np.array_equal(a[f"g{g}_sol{i}.npy"], c.sols[i][rows])


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", *args],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_the_fields(tmp_path, transfer):
    from parmmg_amd import _native as N
    d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k, v in HEADLINE.items():
        assert d[k] == v, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    m, x, t, sols, tv = bench.build_case(bench.CONFIGS["C1"], 0)
    # value = vertices of all timed steps / their time, ms_per_step = that time / steps
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(len(x) / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["per_iteration"]["binding_configuration"] is None
    a = _load(tmp_path)
    assert sorted(a) == ["g0_rows.npy"] + [f"g0_sol{i}.npy" for i in range(len(sols))]
    assert np.array_equal(a["g0_rows.npy"], np.arange(len(x)))
    # the same seeded case, stepped in this process: the same fields.  A point
    # within the walk's 1e-6 barycentric tolerance of a face may be answered
    # from either tet (the hint grid keeps any one sample per cell), which
    # moves a value by at most 1e-6 of the field's range
    transfer.upload_background(m, sols, 0)
    transfer.upload_points(x, t, tets_mmg=tv)
    transfer.run(flags=N.RUN_FRESH_BACKGROUND)
    r = transfer.download(sols_only=True)
    for i, s in enumerate(r.sols):
        got = a[f"g0_sol{i}.npy"]
        assert got.dtype == np.float64 and got.shape == s.shape and np.isfinite(got).all()
        assert np.abs(got - s).max() <= 1e-6 * np.ptp(sols[i][1:])


@pytest.mark.gpu
def test_full_run_reports_the_other_legs():
    d = _bench("--steps", "2", "--warmup", "1", "--full")
    for k, v in HEADLINE.items():
        assert d[k] == v, k
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["per_iteration"]["binding_configuration"]["ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["pcie_inclusive"]["binding_cycle"]["value"] > 0
