#!/usr/bin/env python3
"""A split's new groups as backgrounds: pmx_split_adopt against the path it
replaces, measured in one build.

For each configuration (bench.py's C2 / C3 background, its metric and fields
uploaded) and each number of z-slab parts, summed over the groups and over
--runs runs (median, min, max):

  adopt      pmx_split_adopt of every group into one receiving context, surface
             included: its device time (pmx_kernel_ms 21) and its wall time
  replaced   pmx_split_fetch with the rows, pmx_build_bdry on the fetched tets
             and adjacency, pmx_upload_background with adja = NULL into another
             context: wall time, and the three parts on their own

Before the timed runs the surface of group 0 is compared between the two
receiving contexts (pmx_download_surface).  The device memory the two
receiving contexts hold after the runs is read from the driver (free memory
before they exist and at the end).  One JSON file (--out, default
profiles/split_adopt_bench.json).

  python tools/bench_split_adopt.py [--cases C3:8,C3:100,C2:8] [--runs 3]
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


def background(cfg: dict):
    """bench.build_case's background mesh and solutions (no new points)."""
    from parmmg_amd import mesh as M
    m = M.kuhn_cube(cfg["n"], seed=20250117)
    sols = [M.on_vertices(m, M.shock_metric if cfg["metric"] == "ani" else M.iso_metric)]
    if "ls" in cfg["fields"]:
        sols.append(M.on_vertices(m, M.level_set))
    if "vel" in cfg["fields"]:
        sols.append(M.on_vertices(m, M.velocity))
    return m, sols


def free_bytes():
    """Free device memory as the HIP runtime reports it (the library's own
    runtime: it is loaded with libpmx_transfer.so)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C3:8,C3:100,C2:8")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_adopt_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_split_adopt {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer
    res = {"runs": args.runs, "cases": []}
    src = Transfer(0)
    res["device"] = src.device_info()

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    def replaced(up, g):
        """fetch + pmx_build_bdry + upload of group g: (fetch, bdry, upload) seconds."""
        t0 = time.perf_counter()
        grp = src.split_fetch(g)
        t1 = time.perf_counter()
        npg = grp["xyz"].shape[0] - 1
        tria, adjt = up.build_bdry(grp["tetra_v"], npg, grp["adja"])
        t2 = time.perf_counter()
        up.upload_background(M.Mesh(grp["xyz"], grp["tetra_v"], grp["adja"], tria, adjt), grp["sols"], 0, adja=False)
        t3 = time.perf_counter()
        return t1 - t0, t2 - t1, t3 - t2

    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    loaded = None
    for cname, nparts in cases:
        if loaded != cname:
            phase(f"background {cname}")
            m, sols = background(bench.CONFIGS[cname])
            src.upload_background(m, sols, 0)
            loaded = cname
        part = z_slabs(m, nparts)
        phase(f"{cname} {nparts} parts")
        p = src.split_groups(part, nparts)
        free0 = free_bytes()
        dst, up = Transfer(0), Transfer(0)
        try:
            # warm-up (allocations) and the equality check on group 0
            for g in range(nparts):
                src.split_adopt(g, dst)
            src.split_adopt(0, dst)
            replaced(up, 0)
            (ta, aa), (tb, ab) = dst.download_surface(), up.download_surface()
            assert ta.tobytes() == tb.tobytes() and aa.tobytes() == ab.tobytes(), "surfaces differ"
            nt0 = ta.shape[0] - 1
            for g in range(1, nparts):
                replaced(up, g)
            held = free0 - free_bytes()
            dev, wall, rep, fetch, bdry, upload = [], [], [], [], [], []
            for _ in range(args.runs):
                src.synchronize()
                d = w = 0.0
                for g in range(nparts):
                    t0 = time.perf_counter()
                    src.split_adopt(g, dst)
                    w += time.perf_counter() - t0
                    d += dst.kernel_ms(21)
                dev.append(d)
                wall.append(w * 1e3)
                parts = np.array([replaced(up, g) for g in range(nparts)]).sum(axis=0) * 1e3
                fetch.append(parts[0]); bdry.append(parts[1]); upload.append(parts[2])
                rep.append(float(parts.sum()))
            case = {"config": cname, "parts": nparts, "ne": m.ne, "np": m.np, "solution_doubles": int(sum(src.sizes)),
                    "points_total": int(p["sizes"][:, 1].sum()), "surface_equal_group0": True, "nt_group0": nt0,
                    "adopt_device_ms": summary(dev), "adopt_wall_ms": summary(wall),
                    "replaced_wall_ms": summary(rep), "replaced_fetch_ms": summary(fetch),
                    "replaced_build_bdry_ms": summary(bdry), "replaced_upload_ms": summary(upload),
                    "receiving_contexts_device_bytes": held}
            case["replaced_over_adopt_wall"] = case["replaced_wall_ms"]["median"] / case["adopt_wall_ms"]["median"]
        finally:
            dst.close()
            up.close()
        phase(json.dumps(case))
        res["cases"].append(case)
        flush()
    src.split_release()
    src.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {"config": c["config"], "parts": c["parts"], "adopt_wall_ms": c["adopt_wall_ms"]["median"],
         "replaced_wall_ms": c["replaced_wall_ms"]["median"]} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
