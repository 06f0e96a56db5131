#!/usr/bin/env python3
"""The displacement's tail on the device (pmx_moveifc_fix, pmx_reach_face_marks,
pmx_moveifc_reach, pmx_moveifc_part(NULL)), measured.

For each configuration (bench.py's C2 / C3): rank 1 of 3 holds 8 z-slab old
groups (colours 3 i + 1); rank 0 and rank 2 have one group each (colours 0 and
2), lighter than every local one.  Before each of the two layers the points of
the bottom face are fed colour 0 and those of the top face colour 2, so that
two layers of foreign tets grow on the two interfaces; the entries of the face
communicator are the boundary tets of the bottom and the top cell layer, and
each neighbour reports the colour of an entry's tet when it is its own.  Two
variants: "common" (every foreign piece is reached) and "planted" (before the
second layer --planted interior points are fed colour 0 as well: their balls
become foreign pieces no entry reaches).

First the device's marks after the fix and after the check, both counters and
the check's stats are asserted equal to the CPU twin's (tests/c/reach_ref.c);
no time is reported otherwise.  Then, over --runs runs (median, min, max), each
from the same state after the layers: the device time of pmx_moveifc_fix
(pmx_kernel_ms 23) and of pmx_moveifc_reach (22), the wall time of the new tail
(fix, face marks, check, part with mark = NULL) and of each of its four calls;
and the same tail without the in-place calls: pmx_moveifc_marks,
pmx_fix_contiguity on the host array, the twin's check on one core,
pmx_moveifc_part(mark).  One JSON file (--out, default
profiles/reach_bench.json).

  python tools/bench_reach.py [--configs C2,C3] [--planted 1000] [--runs 3]
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

NLAYERS, NSLABS, NPROCS, MYRANK = 2, 8, 3, 1


def summary(v: list[float]) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--planted", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_reach {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    import moveifc_ref as F
    import reach_ref as X
    from bench_moveifc import z_slabs
    from parmmg_amd import _native as N
    from parmmg_amd.transfer import Transfer
    F.lib()
    X.lib()
    res = {"runs": args.runs, "layers": NLAYERS, "cases": []}
    if os.path.exists(args.out):                    # one configuration per call adds to the file
        with open(args.out) as fh:
            old = json.load(fh)
        res["cases"] = [c for c in old.get("cases", []) if c["config"] not in args.configs.split(",")]
    tr = Transfer(0)
    res["device"] = tr.device_info()
    colors = (NPROCS * np.arange(NSLABS) + MYRANK).astype(np.int32)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    for cname in args.configs.split(","):
        cfg = bench.CONFIGS[cname]
        phase(f"build_case {cname}")
        m, x, t, sols, tv = bench.build_case(cfg, 0)
        del x, t, tv
        n = cfg["n"]
        tg = z_slabs(m, NSLABS)
        cnt = np.bincount(tg, minlength=NSLABS)
        # colours 0 | 1 4 .. 22 | 2: the foreign groups lighter than every local one
        mp = {"nprocs": NPROCS, "myrank": MYRANK, "displsgrp": np.array([0, 1, 1 + NSLABS, 2 + NSLABS], np.int32),
              "mapgrp": np.concatenate([[10], cnt + 1000, [20]]).astype(np.int32)}
        z = m.xyz[1:, 2]
        bottom = (np.nonzero(z == 0.0)[0] + 1).astype(np.int32)
        top = (np.nonzero(z == 1.0)[0] + 1).astype(np.int32)
        inner = np.nonzero((z > 0.3) & (z < 0.7))[0] + 1
        planted = np.sort(np.random.default_rng(7).choice(inner, args.planted, replace=False)).astype(np.int32)
        # the entries: the boundary tets of the bottom and the top cell layer
        tz = m.xyz[m.tet[1:], 2].mean(1)
        nb0 = (m.adja[1:4 * m.ne + 1].reshape(m.ne, 4) == 0)
        fi, rank = [], []
        for lay, r in ((tz * n < 1.0, 0), (tz * n > n - 1.0, 2)):
            k = np.nonzero(lay & nb0.any(1))[0]
            fi.append(12 * (k + 1) + 3 * np.argmax(nb0[k], 1))
            rank.append(np.full(len(k), r))
        fi, rank = np.concatenate(fi).astype(np.int32), np.concatenate(rank)
        del tz, nb0

        def feed(obj, layer, variant, set_colors):
            pts = [bottom, top] + ([planted] if variant == "planted" and layer == 1 else [])
            col = [np.zeros(len(bottom), np.int32), np.full(len(top), 2, np.int32),
                   np.zeros(len(planted), np.int32)][:len(pts)]
            set_colors(np.concatenate(pts), np.concatenate(col))

        def displace(variant):
            tr.moveifc_begin(tg, mp)
            for l in range(NLAYERS):
                feed(tr, l, variant, tr.moveifc_set_colors)
                tr.moveifc_layer()

        def honest(sent):
            return np.where(sent % NPROCS == rank, sent, X.UNSET).astype(np.int32)

        tr.upload_background(m, sols, 0)
        for variant in ("common", "planted"):
            phase(f"{cname} {variant}: twin")
            twin = F.Twin(m, tg, mp)
            for l in range(NLAYERS):
                feed(twin, l, variant, twin.set_colors)
                ok, _ = twin.layer()
                assert ok
            w = X.Twin(m, twin.mark)
            del twin
            t0 = time.perf_counter()
            fixed, fst = w.fix(colors)
            twin_fix = (time.perf_counter() - t0) * 1e3
            cin = honest(fixed[fi // 12 - 1])
            t0 = time.perf_counter()
            ok, out, st = w.reach(fi, cin)
            twin_reach = (time.perf_counter() - t0) * 1e3
            assert ok
            phase("device, checked against the twin")
            displace(variant)
            gst = tr.moveifc_fix()
            assert gst["counter"] == fst["counter"], "the fix's counter differs from the twin's"
            assert np.array_equal(tr.moveifc_marks(), fixed), "the marks after the fix differ from the twin's"
            sent = tr.reach_face_marks(None, fi)
            assert np.array_equal(honest(sent), cin)
            rst = tr.moveifc_reach(fi, cin)
            assert all(rst[k] == st[k] for k in X.REACH_FIELDS), "stats differ from the twin's"
            assert np.array_equal(tr.moveifc_marks(), out), "the marks after the check differ from the twin's"
            ngrps = np.diff(mp["displsgrp"]).astype(np.int32)
            fix_dev, reach_dev, tail, base, base_parts, tail_parts = [], [], [], [], [], []
            for _ in range(args.runs):
                displace(variant)
                tr.synchronize()
                # without the in-place calls: marks down, the fix on the host array, the check on one core
                t0 = time.perf_counter()
                mk = tr.moveifc_marks()
                t1 = time.perf_counter()
                fx, _ = tr.fix_contiguity(mk, colors)
                t2 = time.perf_counter()
                w = X.Twin(m, fx)
                w.flag[1:] = np.isin(fx, colors)           # the flags the fix leaves
                w.base.value = 1
                w.st.counter = fst["counter"]
                t3 = time.perf_counter()
                ok, o2, _ = w.reach(fi, honest(fx[fi // 12 - 1]))
                t4 = time.perf_counter()
                p2, _ = tr.moveifc_part(o2, N.GRPSPL_DISTR_TARGET, ngrps)
                t5 = time.perf_counter()
                base.append(((t5 - t0) - (t3 - t2)) * 1e3)   # the twin's set-up is not the caller's
                base_parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3])
                del w
                # the new tail
                tr.synchronize()
                t0 = time.perf_counter()
                tr.moveifc_fix()
                t1 = time.perf_counter()
                fix_dev.append(tr.kernel_ms(23))
                c2 = honest(tr.reach_face_marks(None, fi))
                t2 = time.perf_counter()
                tr.moveifc_reach(fi, c2)
                t3 = time.perf_counter()
                reach_dev.append(tr.kernel_ms(22))
                p1, _ = tr.moveifc_part(None, N.GRPSPL_DISTR_TARGET, ngrps)
                t4 = time.perf_counter()
                tail.append((t4 - t0) * 1e3)
                tail_parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3])
                assert np.array_equal(p1, p2), "the two tails give different partitions"
            parts, tparts = np.array(base_parts), np.array(tail_parts)
            case = {"config": cname, "variant": variant, "ne": m.ne, "np": m.np, "entries": len(fi),
                    "planted_points": args.planted if variant == "planted" else 0, "equals_twin": True,
                    "fix_stats": gst, "reach_stats": rst, "rounds": rst["rounds"], "relabels": rst["relabels"],
                    "fix_device_ms": summary(fix_dev), "reach_device_ms": summary(reach_dev),
                    "tail_wall_ms": summary(tail), "baseline_wall_ms": summary(base),
                    "tail_fix_wall_ms": summary(list(tparts[:, 0])),
                    "tail_face_marks_wall_ms": summary(list(tparts[:, 1])),
                    "tail_reach_wall_ms": summary(list(tparts[:, 2])),
                    "tail_part_wall_ms": summary(list(tparts[:, 3])),
                    "baseline_marks_download_ms": summary(list(parts[:, 0])),
                    "baseline_fix_host_array_ms": summary(list(parts[:, 1])),
                    "baseline_twin_reach_one_core_ms": summary(list(parts[:, 2])),
                    "baseline_part_ms": summary(list(parts[:, 3])),
                    "twin_one_core_fix_ms": twin_fix, "twin_one_core_reach_ms": twin_reach}
            case["baseline_over_tail"] = case["baseline_wall_ms"]["median"] / case["tail_wall_ms"]["median"]
            case["twin_reach_over_reach_device"] = (case["baseline_twin_reach_one_core_ms"]["median"] /
                                                    case["reach_device_ms"]["median"])
            phase(json.dumps(case))
            res["cases"].append(case)
            flush()
        tr.moveifc_release()
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {k: c.get(k) for k in ("config", "variant", "equals_twin", "rounds", "relabels", "baseline_over_tail")} |
        {"fix_device_ms": c["fix_device_ms"]["median"], "reach_device_ms": c["reach_device_ms"]["median"],
         "tail_wall_ms": c["tail_wall_ms"]["median"], "baseline_wall_ms": c["baseline_wall_ms"]["median"]}
        for c in res["cases"]]}))


if __name__ == "__main__":
    main()
