#!/usr/bin/env python3
"""The device group split (pmx_split_groups / pmx_split_fetch), measured.

For each configuration (bench.py's C2 / C3, its metric and fields uploaded) and
each number of z-slab parts: the plan's device time (pmx_kernel_ms 14), the
wall time of the plan, of the plan plus every group's fetch without and with
the xyz / solution rows, over --runs runs (median, min, max); and once the CPU
twin (tests/c/split_ref.c, one core, integer arrays only), the yardstick: the
reference fills the groups on one core per rank.  The first group's integer
arrays are compared with the twin's.  One JSON file (--out, default
profiles/split_bench.json).

  python tools/bench_split.py [--configs C2,C3] [--parts 8,100] [--runs 3] [--no-twin]
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
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_split {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    from parmmg_amd.transfer import Transfer
    res = {"runs": args.runs, "cases": []}
    tr = Transfer(0)
    res["device"] = tr.device_info()

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for cname in args.configs.split(","):
        cfg = bench.CONFIGS[cname]
        phase(f"build_case {cname}")
        m, x, t, sols, tv = bench.build_case(cfg, 0)
        tr.upload_background(m, sols, 0)
        for nparts in (int(v) for v in args.parts.split(",")):
            part = z_slabs(m, nparts)
            phase(f"{cname} {nparts} parts")
            tr.split_groups(part, nparts)                    # warm-up: allocations
            dev, plan, ints, full = [], [], [], []
            for _ in range(args.runs):
                tr.synchronize()
                t0 = time.perf_counter()
                p = tr.split_groups(part, nparts)
                t1 = time.perf_counter()
                dev.append(tr.kernel_ms(14))
                for g in range(nparts):
                    tr.split_fetch(g, data=False)
                t2 = time.perf_counter()
                for g in range(nparts):
                    tr.split_fetch(g, data=True)
                t3 = time.perf_counter()
                plan.append((t1 - t0) * 1e3)
                ints.append((t2 - t0) * 1e3)
                full.append((t1 - t0 + t3 - t2) * 1e3)
            case = {"config": cname, "parts": nparts, "ne": m.ne, "np": m.np, "solution_doubles": int(sum(tr.sizes)),
                    "points_total": int(p["sizes"][:, 1].sum()), "faces_total": int(p["sizes"][:, 2].sum()),
                    "nodes_total": int(p["sizes"][:, 3].sum()),
                    "plan_device_ms": summary(dev), "plan_wall_ms": summary(plan),
                    "plan_and_fetch_wall_ms": summary(ints), "plan_and_fetch_with_rows_wall_ms": summary(full)}
            if not args.no_twin:
                import split_ref
                split_ref.lib()
                ref = split_ref.split(m, part, nparts)
                case["twin_one_core_ms"] = ref["seconds"] * 1e3       # the C call alone
                g0 = tr.split_fetch(0, data=False)
                case["equals_twin"] = bool(
                    np.array_equal(p["sizes"], ref["sizes"]) and np.array_equal(p["tet_new"], ref["tet_new"]) and
                    all(np.array_equal(g0[k], ref["groups"][0][k]) for k in split_ref.INT_KEYS))
                case["twin_over_plan_and_fetch"] = case["twin_one_core_ms"] / case["plan_and_fetch_wall_ms"]["median"]
                del ref
            phase(json.dumps(case))
            res["cases"].append(case)
            flush()
        tr.split_release()
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {k: c.get(k) for k in ("config", "parts", "equals_twin")} | {"plan_device_ms": c["plan_device_ms"]["median"]}
        for c in res["cases"]]}))


if __name__ == "__main__":
    main()
