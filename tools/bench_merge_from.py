#!/usr/bin/env python3
"""The merge from held groups (pmx_merge_groups_from) against the merge from
host views (pmx_merge_groups), measured in one build on one device.

For each configuration (bench.py's C2 / C3, its metric and fields) and each
number of z-slab groups: the groups are made by the device split of the mesh;
every group becomes the background of a context of its own (pmx_split_adopt,
one context per group -- at 100 groups too: the holders of C3 take 2.8 GB
together, so none is reused) and is also fetched to the host.  First the
outputs of the held merge -- sizes, every array of the fetch, the maps of the
first and the last group -- are asserted equal to those of the host-source
merge; no time is reported otherwise.  Then, over --runs rounds after one
warm-up (median, min, max), the two paths alternating within a round: the
plan's device time (pmx_kernel_ms 16), the plan's wall time, the wall time of
plan + adopt.  Device memory (hipMemGetInfo): what the holders take (the
difference around their creation, the split plan allocated at both ends), and
the peak in use while a plan is made with the holders alive -- a thread samples
hipMemGetInfo as fast as it can during the call; the peak is the largest
sample, reported as it is and above the level just before the call.

--unpacked P: on the first group count also the held merge of the same groups
with P percent more points that no tet names and P percent more tets deleted,
spread evenly (uploaded holders): what the mark pass and the scans cost when
they have something to drop.

One JSON file (--out, default profiles/merge_from_bench.json).

  python tools/bench_merge_from.py [--configs C2,C3] [--parts 8,100] [--runs 5] [--unpacked 5]
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

IDX = ("node_index1", "node_index2", "face_index1", "face_index2")


def summary(v: list[float]) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def z_slabs(m, nparts: int) -> np.ndarray:
    z = m.xyz[:, 2]
    t = m.tet[1:]
    zc = (z[t[:, 0]] + z[t[:, 1]] + z[t[:, 2]] + z[t[:, 3]]) * 0.25
    return np.minimum((zc * nparts).astype(np.int32), nparts - 1)


def used_bytes() -> int:
    """Device memory in use (hipMemGetInfo of the runtime the library has loaded)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(total.value - free.value)


class Peak:
    """The largest hipMemGetInfo sample taken by a thread while the block runs."""

    def __enter__(self):
        import threading
        self.before = self.peak = used_bytes()
        self.samples, self._stop = 0, False

        def run():
            while not self._stop:
                self.peak = max(self.peak, used_bytes())
                self.samples += 1
        self._t = threading.Thread(target=run)
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        self._t.join()
        self.peak = max(self.peak, used_bytes())
        return False


def blob(tr, ngrp):
    d = tr.merge_fetch()
    out = {k: v for k, v in d.items() if k != "sols"}
    for i, a in enumerate(d["sols"]):
        out[f"sol{i}"] = a[1:]
    out["xyz"] = out["xyz"][1:]
    for g in (0, ngrp - 1):
        out[f"pn{g}"], out[f"tn{g}"] = tr.merge_maps(g)
    return out


def timed(tr, runs, plans: dict) -> dict:
    """plans: name -> callable; every round runs each once, in turn."""
    acc = {k: ([], [], []) for k in plans}
    for _ in range(runs):
        for k, plan in plans.items():
            tr.synchronize()
            t0 = time.perf_counter()
            plan()
            t1 = time.perf_counter()
            acc[k][0].append(tr.kernel_ms(16))
            tr.merge_adopt(0)
            t2 = time.perf_counter()
            acc[k][1].append((t1 - t0) * 1e3)
            acc[k][2].append((t2 - t0) * 1e3)
    return {k: {"plan_device_ms": summary(d), "plan_wall_ms": summary(w), "plan_and_adopt_wall_ms": summary(b)}
            for k, (d, w, b) in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--parts", default="8,100")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--unpacked", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_from_bench.json"))
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_merge_from {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    import merge_from_ref
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer
    res = {"runs": args.runs, "cases": []}
    if os.path.exists(args.out):               # one configuration per call: keep the others' cases
        with open(args.out) as fh:
            old = json.load(fh)
        res["cases"] = [c for c in old.get("cases", []) if c["config"] not in args.configs.split(",")]
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
        for ip, nparts in enumerate(int(v) for v in args.parts.split(",")):
            phase(f"{cname} {nparts} groups: device split, one holder per group")
            tr.upload_background(m, sols, 0)
            sp = tr.split_groups(z_slabs(m, nparts), nparts)
            groups = [tr.split_fetch(g) for g in range(nparts)]
            before_holders = used_bytes()                        # the split plan is allocated here ...
            holders = [Transfer(0) for _ in range(nparts)]
            for g, h in enumerate(holders):
                tr.split_adopt(g, h, 0, surface=False)
            tr.synchronize()
            holder_bytes = used_bytes() - before_holders         # ... and here
            tr.split_release()
            comm = {"int_node_nitem": sp["int_node_nitem"], "int_face_nitem": sp["int_face_nitem"]}
            held = [dict({k: grp[k] for k in IDX}, held=h) for grp, h in zip(groups, holders)]
            phase("host-source merge (the yardstick), then the held merge, compared")
            sz_host = tr.merge_groups(groups, comm)["sizes"]
            want = blob(tr, nparts)
            tr.merge_adopt(0)
            sz = tr.merge_groups_from(held, comm)["sizes"]
            got = blob(tr, nparts)
            assert np.array_equal(sz, sz_host), "sizes differ from the host-source merge's"
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), k + " differs from the host-source merge's"
            tr.merge_adopt(0)
            # peaks: each path once more from the same state (no plan, the adopted group, the holders alive)
            mem = {}
            for name, plan in (("held", lambda: tr.merge_groups_from(held, comm)),
                               ("host", lambda: tr.merge_groups(groups, comm))):
                tr.merge_release()
                with Peak() as pk:
                    plan()
                mem[name] = {"before_bytes": pk.before, "peak_bytes": pk.peak, "peak_above_before_bytes": pk.peak - pk.before,
                             "kept_bytes": used_bytes() - pk.before, "samples": pk.samples}
            S = int(sum(tr.sizes))
            P, T = int(sum(g["xyz"].shape[0] - 1 for g in groups)), int(m.ne)
            case = {"config": cname, "groups": nparts, "ne": m.ne, "np": m.np, "solution_doubles": S, "points_in": P,
                    "host_bytes_in": P * (24 + 8 * S) + T * 16, "equals_host_source_merge": True,
                    "device_bytes_holders": holder_bytes, "device_memory_during_plan": mem}
            phase("held and host views, alternating")
            case.update(timed(tr, args.runs, {"held": lambda: tr.merge_groups_from(held, comm),
                                              "host": lambda: tr.merge_groups(groups, comm)}))
            for k in ("plan_device_ms", "plan_wall_ms", "plan_and_adopt_wall_ms"):
                case["host_over_held_" + k] = case["host"][k]["median"] / case["held"][k]["median"]
            tr.merge_release()
            for h in holders:
                h.close()
            if ip == 0 and args.unpacked > 0:
                phase(f"{args.unpacked} % unused points and deleted tets: uploaded holders")
                own = []
                for grp in groups:
                    npk, nek = grp["xyz"].shape[0] - 1, grp["tetra_v"].shape[0] - 1
                    hp, ht = int(npk * args.unpacked / 100), int(nek * args.unpacked / 100)
                    own.append(merge_from_ref.unpack_group(
                        grp, np.unique(np.linspace(1, npk + hp, hp).astype(np.int64)) if hp else np.zeros(0, np.int64),
                        np.unique(np.linspace(1, nek + ht, ht).astype(np.int64)) if ht else np.zeros(0, np.int64)))
                holders = []
                for o in own:
                    ne = o["tetra_v"].shape[0] - 1
                    h = Transfer(0)
                    h.upload_background(M.Mesh(o["xyz"], o["tetra_v"], np.zeros(4 * ne + 5, np.int32),
                                               np.zeros((1, 3), np.int32), np.zeros(4, np.int32)), o["sols"], 0, adja=False)
                    holders.append(h)
                uheld = [dict({k: o[k] for k in IDX}, held=h) for o, h in zip(own, holders)]
                sz = tr.merge_groups_from(uheld, comm)["sizes"]
                d = tr.merge_fetch()
                assert np.array_equal(sz, sz_host) and d["tetra_v"].tobytes() == want["tetra_v"].tobytes(), "unpacked"
                assert d["xyz"][1:].tobytes() == want["xyz"].tobytes(), "unpacked: xyz"
                tr.merge_adopt(0)
                case["held_unpacked"] = dict(timed(tr, args.runs, {"u": lambda: tr.merge_groups_from(uheld, comm)})["u"],
                                             percent=args.unpacked,
                                             points_dropped=int(sum(o["xyz"].shape[0] - 1 for o in own)) - P,
                                             tets_dropped=int(sum(o["tetra_v"].shape[0] - 1 for o in own)) - T)
                case["unpacked_over_packed_plan_device_ms"] = (case["held_unpacked"]["plan_device_ms"]["median"] /
                                                               case["held"]["plan_device_ms"]["median"])
                tr.merge_release()
                for h in holders:
                    h.close()
                del own, uheld
            phase(json.dumps(case))
            res["cases"].append(case)
            flush()
            del groups, want, got, held
    tr.close()
    flush()
    print(json.dumps({"out": args.out, "cases": [
        {k: c.get(k) for k in ("config", "groups", "equals_host_source_merge")} |
        {"held_plan_device_ms": c["held"]["plan_device_ms"]["median"],
         "host_plan_device_ms": c["host"]["plan_device_ms"]["median"]} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
