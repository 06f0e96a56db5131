#!/usr/bin/env python3
"""The step from the displacement's marks to the split plan, on the device
(pmx_part_from_marks + pmx_split_groups_part) and through the host's array
(pmx_moveifc_marks + pmx_moveifc_part(mark) + pmx_split_groups(part), whose
PMMG_part_getInterfaces is three single-threaded host loops), measured in one
build on one box.

For each case (bench.py's configuration, number of z-slab old groups): rank 1
of 3 holds the slabs (colours 3 i + 1); rank 0 and rank 2 have one group each
(colours 0 and 2), lighter than every local one, fed to the bottom and the top
face before each of the two layers -- tools/bench_reach.py's "common" variant,
with its face-communicator entries.

Every run starts from the same state after the layers and times, in order: the
three calls both tails share (pmx_moveifc_fix, pmx_reach_face_marks,
pmx_moveifc_reach), then the device path, then the host-array path on the same
marks -- neither path changes them.  A whole tail is the shared calls plus one
path.  Before any time is reported the two plans' sizes and tet_new, the two
partitions and the group counts are asserted equal.  Reported per case, median
(min, max) of --runs runs: pmx_kernel_ms(24), the wall time of each path and of
its calls, and both tails.  One JSON file (--out, default
profiles/part_bench.json); a call with --cases adds to it.

  python tools/bench_part.py [--cases C3:8,C3:100,C2:8] [--runs 3]
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

NLAYERS, NPROCS, MYRANK = 2, 3, 1


def summary(v: list[float]) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3:8,C3:100,C2:8")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_part {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    from bench_moveifc import z_slabs
    from parmmg_amd import _native as N
    from parmmg_amd.transfer import Transfer
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    res = {"runs": args.runs, "layers": NLAYERS, "cases": []}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            old = json.load(fh)
        res["cases"] = [c for c in old.get("cases", []) if (c["config"], c["slabs"]) not in cases]
    tr = Transfer(0)
    res["device"] = tr.device_info()

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    built = None
    for cname, nslabs in cases:
        if built != cname:
            phase(f"build_case {cname}")
            m, x, t, sols, tv = bench.build_case(bench.CONFIGS[cname], 0)
            del x, t, tv
            n = bench.CONFIGS[cname]["n"]
            z = m.xyz[1:, 2]
            bottom = (np.nonzero(z == 0.0)[0] + 1).astype(np.int32)
            top = (np.nonzero(z == 1.0)[0] + 1).astype(np.int32)
            tz = m.xyz[m.tet[1:], 2].mean(1)
            nb0 = (m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) == 0)
            fi, rank = [], []
            for lay, r in ((tz * n < 1.0, 0), (tz * n > n - 1.0, 2)):
                k = np.nonzero(lay & nb0.any(1))[0]
                fi.append(12 * (k + 1) + 3 * np.argmax(nb0[k], 1))
                rank.append(np.full(len(k), r))
            fi, rank = np.concatenate(fi).astype(np.int32), np.concatenate(rank)
            del tz, nb0, z
            tr.upload_background(m, sols, 0)
            built = cname
        tg = z_slabs(m, nslabs)
        cnt = np.bincount(tg, minlength=nslabs)
        mp = {"nprocs": NPROCS, "myrank": MYRANK, "displsgrp": np.array([0, 1, 1 + nslabs, 2 + nslabs], np.int32),
              "mapgrp": np.concatenate([[10], cnt + 1000, [20]]).astype(np.int32)}
        ngrps = np.diff(mp["displsgrp"]).astype(np.int32)
        feed_pts = np.concatenate([bottom, top])
        feed_col = np.concatenate([np.zeros(len(bottom), np.int32), np.full(len(top), 2, np.int32)])

        def honest(sent):
            return np.where(sent % NPROCS == rank, sent, -1).astype(np.int32)

        phase(f"{cname} from {nslabs} slabs")
        dev_ms, plan_ms, common, new, old_, new_parts, old_parts = [], [], [], [], [], [], []
        ngrp = 0
        for run in range(args.runs):
            tr.moveifc_begin(tg, mp)
            for _ in range(NLAYERS):
                tr.moveifc_set_colors(feed_pts, feed_col)
                tr.moveifc_layer()
            tr.synchronize()
            t0 = time.perf_counter()
            tr.moveifc_fix()
            cin = honest(tr.reach_face_marks(None, fi))
            tr.moveifc_reach(fi, cin)
            t1 = time.perf_counter()
            # the device path
            ngrp, gm = tr.part_from_marks(N.GRPSPL_DISTR_TARGET, ngrps)
            t2 = time.perf_counter()
            dev_ms.append(tr.kernel_ms(24))
            t2b = time.perf_counter()
            plan = tr.split_groups_part()
            t3 = time.perf_counter()
            plan_ms.append(tr.kernel_ms(14))
            # the path it replaces: the marks down, the host loops, the array up again
            mk = tr.moveifc_marks()
            t4 = time.perf_counter()
            p2, n2 = tr.moveifc_part(mk, N.GRPSPL_DISTR_TARGET, ngrps)
            t5 = time.perf_counter()
            plan2 = tr.split_groups(p2, n2)
            t6 = time.perf_counter()
            if run == 0:
                assert n2 == ngrp, "the two paths count different groups"
                assert np.array_equal(plan["sizes"], plan2["sizes"]), "the two plans' sizes differ"
                assert np.array_equal(plan["tet_new"], plan2["tet_new"]), "the two plans' tet_new differ"
                tr.part_from_marks(N.GRPSPL_DISTR_TARGET, ngrps)
                assert np.array_equal(tr.part_download()[0], p2), "the two partitions differ"
                assert np.array_equal(gm, mk[np.unique(p2, return_index=True)[1]]), \
                    "group_mark is not the mark of each group's first tet"
            del plan, plan2, mk, p2
            common.append((t1 - t0) * 1e3)
            new.append(((t2 - t1) + (t3 - t2b)) * 1e3)
            new_parts.append([(t2 - t1) * 1e3, (t3 - t2b) * 1e3])
            old_.append((t6 - t3) * 1e3)
            old_parts.append([(t4 - t3) * 1e3, (t5 - t4) * 1e3, (t6 - t5) * 1e3])
        npa, opa = np.array(new_parts), np.array(old_parts)
        case = {"config": cname, "slabs": nslabs, "ne": m.ne, "np": m.np, "ngrp": ngrp, "entries": len(fi),
                "plans_equal": True,
                "part_device_ms": summary(dev_ms),
                "part_split_wall_ms": summary(new),
                "part_from_marks_wall_ms": summary(list(npa[:, 0])),
                "split_groups_part_wall_ms": summary(list(npa[:, 1])),
                "split_plan_device_ms": summary(plan_ms),      # pmx_kernel_ms(14) of split_groups_part
                "host_array_wall_ms": summary(old_),
                "host_marks_download_wall_ms": summary(list(opa[:, 0])),
                "host_moveifc_part_wall_ms": summary(list(opa[:, 1])),
                "host_split_groups_wall_ms": summary(list(opa[:, 2])),
                "shared_fix_marks_reach_wall_ms": summary(common),
                "tail_device_wall_ms": summary([a + b for a, b in zip(common, new)]),
                "tail_host_array_wall_ms": summary([a + b for a, b in zip(common, old_)])}
        case["host_array_over_device"] = case["host_array_wall_ms"]["median"] / case["part_split_wall_ms"]["median"]
        case["tail_host_array_over_device"] = (case["tail_host_array_wall_ms"]["median"] /
                                               case["tail_device_wall_ms"]["median"])
        case["part_device_gbs"] = 12.0 * m.ne / (case["part_device_ms"]["median"] * 1e-3) / 1e9
        phase(json.dumps(case))
        res["cases"].append(case)
        flush()
        tr.moveifc_release()
        tr.split_release()
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {"config": c["config"], "slabs": c["slabs"], "part_device_ms": c["part_device_ms"]["median"],
         "part_split_wall_ms": c["part_split_wall_ms"]["median"], "host_array_wall_ms": c["host_array_wall_ms"]["median"],
         "tail_device_wall_ms": c["tail_device_wall_ms"]["median"],
         "tail_host_array_wall_ms": c["tail_host_array_wall_ms"]["median"]} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
