#!/usr/bin/env python3
"""The device interface displacement (pmx_moveifc_begin / _layer / _marks), measured.

For each configuration (bench.py's C2 / C3) and each number of z-slab old
groups: the weights are the slabs' tet counts plus the slab's rank from the
end of the tet numbering, so that the lighter groups come later in the
numbering and the front is not empty.  First the device's marks, tmp, s, front
and negrp after begin and after each of the two layers are asserted equal to
the CPU twin's (tests/c/moveifc_ref.c); no time is reported otherwise.  Then,
over --runs runs after that warm-up (median, min, max): the device time of
begin (pmx_kernel_ms 19) and of each layer (20), the download of the marks, the
wall time of the whole sequence with host arrays in and out; and what a caller
pays today: the twin on one core (the C calls alone, once).  One JSON file
(--out, default profiles/moveifc_bench.json).

  python tools/bench_moveifc.py [--configs C2,C3] [--parts 8,100] [--runs 3]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

NLAYERS = 2


def summary(v: list[float]) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def z_slabs(m, nparts: int) -> np.ndarray:
    z = m.xyz[:, 2]
    t = m.tet[1:]
    zc = (z[t[:, 0]] + z[t[:, 1]] + z[t[:, 2]] + z[t[:, 3]]) * 0.25
    return np.minimum((zc * nparts).astype(np.int32), nparts - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--parts", default="8,100")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moveifc_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_moveifc {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    import moveifc_ref as F
    from parmmg_amd.transfer import Transfer
    F.lib()
    res = {"runs": args.runs, "layers": NLAYERS, "cases": []}
    tr = Transfer(0)
    res["device"] = tr.device_info()

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    def same(t, what):
        tmp, s, front = tr.moveifc_points()
        negrp, _ = tr.moveifc_groups()
        for k, a in (("mark", tr.moveifc_marks()), ("tmp", tmp), ("s", s), ("front", front), ("negrp", negrp)):
            assert np.array_equal(a, getattr(t, k)), f"{k} differs from the twin's {what}"

    for cname in args.configs.split(","):
        cfg = bench.CONFIGS[cname]
        phase(f"build_case {cname}")
        m, x, t, sols, tv = bench.build_case(cfg, 0)
        del x, t, tv
        for nparts in (int(v) for v in args.parts.split(",")):
            tg = z_slabs(m, nparts)
            cnt = np.bincount(tg, minlength=nparts)
            where = np.bincount(tg, weights=np.arange(m.ne), minlength=nparts) / np.maximum(cnt, 1)
            rank = np.empty(nparts, np.int64)
            rank[np.argsort(-where)] = np.arange(nparts)      # 0: the slab last in the numbering
            mp = F.single_map(cnt + rank)
            phase(f"{cname} {nparts} groups: twin")
            t0 = time.perf_counter()
            twin = F.Twin(m, tg, mp)
            twin_begin = (time.perf_counter() - t0) * 1e3
            phase("device, checked against the twin")
            tr.upload_background(m, sols, 0)
            nfront = tr.moveifc_begin(tg, mp)
            assert nfront == twin.nfront > 0, "the front differs from the twin's, or is empty"
            same(twin, "after begin")
            twin_layers, stats = [], []
            for l in range(NLAYERS):
                t0 = time.perf_counter()
                ok, st = twin.layer()
                twin_layers.append((time.perf_counter() - t0) * 1e3)
                got = tr.moveifc_layer()
                assert ok and all(got[k] == st[k] for k in st if k in got), "stats differ from the twin's"
                same(twin, f"after layer {l}")
                stats.append(got)
            begin_dev, layer_dev, marks_ms, wall = [], [[] for _ in range(NLAYERS)], [], []
            for _ in range(args.runs):
                tr.synchronize()
                t0 = time.perf_counter()
                tr.moveifc_begin(tg, mp)
                begin_dev.append(tr.kernel_ms(19))
                for l in range(NLAYERS):
                    tr.moveifc_layer()
                    layer_dev[l].append(tr.kernel_ms(20))
                t1 = time.perf_counter()
                tr.moveifc_marks()
                t2 = time.perf_counter()
                marks_ms.append((t2 - t1) * 1e3)
                wall.append((t2 - t0) * 1e3)
            tr.moveifc_release()
            case = {"config": cname, "groups": nparts, "ne": m.ne, "np": m.np, "equals_twin": True,
                    "nfront": nfront, "layer_stats": stats,
                    "begin_device_ms": summary(begin_dev),
                    "layer_device_ms": [summary(v) for v in layer_dev],
                    "marks_download_ms": summary(marks_ms), "whole_wall_ms": summary(wall),
                    "twin_one_core_begin_ms": twin_begin, "twin_one_core_layer_ms": twin_layers}
            case["twin_one_core_ms"] = twin_begin + sum(twin_layers)
            case["twin_over_whole_wall"] = case["twin_one_core_ms"] / case["whole_wall_ms"]["median"]
            phase(json.dumps(case))
            res["cases"].append(case)
            flush()
            del twin
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {k: c.get(k) for k in ("config", "groups", "equals_twin", "twin_over_whole_wall")} |
        {"begin_device_ms": c["begin_device_ms"]["median"],
         "layer_device_ms": [v["median"] for v in c["layer_device_ms"]]} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
