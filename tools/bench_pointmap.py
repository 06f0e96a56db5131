#!/usr/bin/env python3
"""Point-map starts (PMX_RUN_POINTMAP) against the hint grids, measured.

For each configuration (bench.py's C2 / C3) and background tet numbering (the
generator's lattice order, "lex", and the shuffled one) the same context runs
plain and flagged steps alternately, both PMX_RUN_FRESH_BACKGROUND (one ParMmg
iteration per step: the flagged step rebuilds the first-incident-element maps,
the plain one the hint grids).  Sources are the nearest lattice vertex of each
new point, computed from the generator's layout (vertex (i, j, k) of the
(n+1)^3 lattice is 1 + i + (n+1) (j + (n+1) k); a numbering permutes tets only).

Per mode: wall ms/step and the per-kernel event times (medians over the
interleaved steps, with the min-max range), mean / max walk steps and the
exhaustive searches; for the flagged mode the map build's ms and the atomics
it issued.  One JSON file (--out, default profiles/pointmap_bench.json).

--baseline-lib PATH: also interleave the plain C3 step of another build of
libpmx_transfer.so (the parent commit's) with this one's in the same process,
for the "default step unchanged" A/B -- on a context of each library created
one after the other, and on the context the cases ran on.

  python tools/bench_pointmap.py [--configs C2,C3] [--numberings lex,shuffle]
                                 [--steps 20] [--warmup 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KERNELS = ["hint", "vol", "bdy", "exhaustive", "total", "derive", "pointmap_maps"]


def lattice_sources(n: int, x: np.ndarray) -> np.ndarray:
    ijk = np.clip(np.rint(x * n).astype(np.int64), 0, n)
    n1 = n + 1
    return (1 + ijk[:, 0] + n1 * (ijk[:, 1] + n1 * ijk[:, 2])).astype(np.int32)


def summary(v: list[float]) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def timed_step(tr, flags: int, pointmap: bool, nk: int) -> tuple[float, list[float]]:
    tr.timing_reset()
    tr.synchronize()
    t0 = time.perf_counter()
    tr.run(timing=True, flags=flags, pointmap=pointmap)
    tr.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, [tr.kernel_ms(i) for i in range(nk)]


def fold(walls, ks, names) -> dict:
    out = {"ms_per_step": summary(walls)}
    for i, name in enumerate(names):
        out[name + "_ms"] = summary([k[i] for k in ks])
    return out


def transfer_on(lib_path: str, device: int):
    """A Transfer over another build of the library (symbols it lacks are left out)."""
    from parmmg_amd import _native as N
    from parmmg_amd.transfer import Transfer
    lib = C.CDLL(lib_path)
    for name, (res, args) in N.SIGNATURES.items():
        f = getattr(lib, name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
    t = Transfer.__new__(Transfer)
    t._peer, t.device, t.lib = None, device, lib
    t.ctx = lib.pmx_create(device)
    if not t.ctx:
        raise RuntimeError("pmx_create failed on the baseline library")
    t._keep, t.sizes, t.npts, t.n_new_tets = [], [], 0, 0
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--numberings", default="lex,shuffle")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointmap_bench.json"))
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_pointmap {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    from parmmg_amd import _native as N
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer
    FRESH = N.RUN_FRESH_BACKGROUND
    res = {"steps": args.steps, "warmup": args.warmup, "flags": "PMX_RUN_FRESH_BACKGROUND both modes",
           "sources": "nearest lattice vertex", "cases": []}
    tr = Transfer(0)
    res["device"] = tr.device_info()
    for cname in args.configs.split(","):
        cfg = bench.CONFIGS[cname]
        phase(f"build_case {cname}")
        m0, x, t, sols, tv = bench.build_case(cfg, 0)
        src = lattice_sources(cfg["n"], x)
        for numb in args.numberings.split(","):
            phase(f"{cname} numbering {numb}")
            m = M.numbering(m0, numb)[0]
            tr.upload_background(m, sols, 0)
            tr.upload_points(x, t, tets_mmg=tv)
            tr.upload_point_sources(src)
            for _ in range(args.warmup):
                tr.run(flags=FRESH)
                tr.run(flags=FRESH, pointmap=True)
            tr.synchronize()
            w = {False: [], True: []}
            k = {False: [], True: []}
            for _ in range(args.steps):
                for pm in (False, True):
                    a, b = timed_step(tr, FRESH, pm, len(KERNELS))
                    w[pm].append(a)
                    k[pm].append(b)
            case = {"config": cname, "numbering": numb, "ne": m.ne, "np": m.np, "new_points": len(x)}
            for pm, key in ((False, "grid"), (True, "pointmap")):
                tr.run(flags=FRESH, pointmap=pm)
                st = tr.locate_stats()
                d = fold(w[pm], k[pm], KERNELS)
                d.update(stepav=st["stepav"], stepmax=st["stepmax"], nexhaust=st["nexhaust"],
                         nclosest=st["nclosest"])
                if pm:
                    d.update(tr.pointmap_stats(), atomic_candidates_tets=4 * m.ne,
                             atomic_candidates_trias=3 * m.nt)
                case[key] = d
            g, p = case["grid"]["ms_per_step"]["median"], case["pointmap"]["ms_per_step"]["median"]
            case["pointmap_over_grid"] = p / g
            phase(f"{cname} {numb}: grid {g:.3f} ms, point-map {p:.3f} ms "
                  f"(maps {case['pointmap']['pointmap_maps_ms']['median']:.3f} ms)")
            res["cases"].append(case)
            if args.baseline_lib and cname == "C3" and numb == "lex":
                phase("baseline library A/B (plain C3 step)")
                # three contexts: the baseline library's, one of this library
                # created the same way right after it (the control: a context's
                # buffers land where the allocator puts them, and the step's
                # time follows), and the one the cases above ran on
                tb = transfer_on(args.baseline_lib, 0)
                tc = Transfer(0)
                for T in (tb, tc):
                    T.upload_background(m, sols, 0)
                    T.upload_points(x, t, tets_mmg=tv)
                for _ in range(args.warmup):
                    for T in (tb, tc, tr):
                        T.run(flags=FRESH)
                wa = {"baseline": [], "this_fresh_context": [], "this": []}
                ka = {"baseline": [], "this_fresh_context": [], "this": []}
                for _ in range(args.steps):
                    for name, T in (("baseline", tb), ("this_fresh_context", tc), ("this", tr)):
                        T.timing_reset()
                        T.synchronize()
                        t0 = time.perf_counter()
                        T.run(timing=True, flags=FRESH)
                        T.synchronize()
                        wa[name].append((time.perf_counter() - t0) * 1e3)
                        ka[name].append([T.kernel_ms(i) for i in range(6)])
                ab = {name: fold(wa[name], ka[name], KERNELS[:6]) for name in wa}
                ab["this_fresh_context_minus_baseline_total_ms"] = (
                    ab["this_fresh_context"]["total_ms"]["median"] - ab["baseline"]["total_ms"]["median"])
                res["plain_c3_vs_baseline"] = ab
                phase("A/B total ms, median [min, max]: " + ", ".join(
                    f"{name} {ab[name]['total_ms']['median']:.4f} [{ab[name]['total_ms']['min']:.4f}, "
                    f"{ab[name]['total_ms']['max']:.4f}]" for name in wa))
                tb.close()
                tc.close()
    tr.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": args.out, "cases": [
        {k: c[k] for k in ("config", "numbering", "pointmap_over_grid")} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
