#!/usr/bin/env python3
"""The device group merge (pmx_merge_groups / _fetch / _adopt), measured.

For each configuration (bench.py's C2 / C3, its metric and fields) and each
number of z-slab groups: the groups are made by the device split of the mesh
(pmx_split_groups / pmx_split_fetch, whose output the split's tests pin to its
twin) and merged back.  First the device's outputs -- sizes, every array of
the fetch, the maps of the first and the last group -- are asserted equal to
the CPU twin's (tests/c/merge_ref.c); no time is reported otherwise.  Then,
over --runs runs after one warm-up (median, min, max): the plan's device time
(pmx_kernel_ms 16), the wall time of the plan with the host arrays going in, of
the plan plus the fetch of everything, of the plan plus the adopt; and what a
caller pays today: the twin on one core (the C call alone, once) plus
pmx_upload_background of its result.  One JSON file (--out, default
profiles/merge_bench.json).

  python tools/bench_merge.py [--configs C2,C3] [--parts 8,100] [--runs 3]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_merge {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    import merge_ref
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer
    merge_ref.lib()
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
        for nparts in (int(v) for v in args.parts.split(",")):
            phase(f"{cname} {nparts} groups: device split")
            tr.upload_background(m, sols, 0)
            sp = tr.split_groups(z_slabs(m, nparts), nparts)
            groups = [tr.split_fetch(g) for g in range(nparts)]
            tr.split_release()
            comm = {"int_node_nitem": sp["int_node_nitem"], "int_face_nitem": sp["int_face_nitem"]}
            phase("twin")
            ref = merge_ref.merge(groups, comm)
            phase("device, checked against the twin")
            sz = tr.merge_groups(groups, comm)["sizes"]          # also the warm-up: allocations
            got = tr.merge_fetch()
            assert np.array_equal(sz, ref["sizes"]), "sizes differ from the twin's"
            for k in merge_ref.INT_KEYS:
                assert np.array_equal(got[k], ref[k]), k + " differs from the twin's"
            assert got["xyz"][1:].tobytes() == ref["xyz"][1:].tobytes(), "xyz differs from the twin's"
            for a, b in zip(got["sols"], ref["sols"]):
                assert a[1:].tobytes() == b[1:].tobytes(), "solution rows differ from the twin's"
            for g in (0, nparts - 1):
                pn, tn = tr.merge_maps(g)
                assert np.array_equal(pn, ref["maps"][g][0]) and np.array_equal(tn, ref["maps"][g][1]), "maps differ"
            tr.merge_adopt(0)                                    # warm-up of the adopt's buffers
            dev, plan, fetch, adopt, adopt_dev = [], [], [], [], []
            for _ in range(args.runs):
                tr.synchronize()
                t0 = time.perf_counter()
                tr.merge_groups(groups, comm)
                t1 = time.perf_counter()
                dev.append(tr.kernel_ms(16))
                tr.merge_fetch()
                t2 = time.perf_counter()
                tr.merge_adopt(0)
                t3 = time.perf_counter()
                adopt_dev.append(tr.kernel_ms(18))
                plan.append((t1 - t0) * 1e3)
                fetch.append((t2 - t0) * 1e3)
                adopt.append((t1 - t0 + t3 - t2) * 1e3)
            tr.merge_release()
            phase("upload of the twin's result")
            ne = int(ref["sizes"][1])
            mm = M.Mesh(ref["xyz"], ref["tetra_v"], np.zeros(4 * ne + 5, np.int32), np.zeros((1, 3), np.int32),
                        np.zeros(4, np.int32))
            tr.upload_background(mm, ref["sols"], 0, adja=False)
            up = []
            for _ in range(args.runs):
                tr.synchronize()
                t0 = time.perf_counter()
                tr.upload_background(mm, ref["sols"], 0, adja=False)
                up.append((time.perf_counter() - t0) * 1e3)
            case = {"config": cname, "groups": nparts, "ne": m.ne, "np": m.np, "solution_doubles": int(sum(tr.sizes)),
                    "points_in": int(sum(g["xyz"].shape[0] - 1 for g in groups)),
                    "node_entries_in": int(sum(len(g["node_index1"]) for g in groups)),
                    "face_entries_in": int(sum(len(g["face_index1"]) for g in groups)),
                    "equals_twin": True,
                    "plan_device_ms": summary(dev), "plan_wall_ms": summary(plan),
                    "plan_and_fetch_wall_ms": summary(fetch), "plan_and_adopt_wall_ms": summary(adopt),
                    "adopt_device_ms": summary(adopt_dev),
                    "twin_one_core_ms": ref["seconds"] * 1e3, "upload_of_twin_result_wall_ms": summary(up)}
            case["today_ms"] = case["twin_one_core_ms"] + case["upload_of_twin_result_wall_ms"]["median"]
            case["today_over_plan_and_adopt"] = case["today_ms"] / case["plan_and_adopt_wall_ms"]["median"]
            phase(json.dumps(case))
            res["cases"].append(case)
            flush()
            del groups, ref, got, mm
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {k: c.get(k) for k in ("config", "groups", "equals_twin")} | {"plan_device_ms": c["plan_device_ms"]["median"]}
        for c in res["cases"]]}))


if __name__ == "__main__":
    main()
