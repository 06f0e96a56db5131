#!/usr/bin/env python3
"""More solution fields than the fused step carries (pmx_interp_more), measured.

For each configuration (bench.py's C3 / C2 inputs) the step carries the
metric + 4 fields; 8 and 16 extra scalar fields then go through
Transfer.interp_more on the same context.  Everything is interleaved in one
process: warm-up, then at least --steps timed rounds; medians with min-max.

a. batch cost -- the batch kernels' event time (pmx_kernel_ms 7) per batch of
   8 scalars and the bytes a batch moves at least (per located point: list
   entry, coordinates, kind, element, status, the 32-B tet record, 4 vertices
   of 24 B, 4 rows of 64 B, the 64-B output row and the mask byte), against the
   yardstick: k_walks (pmx_kernel_ms 1) on the same build and input with 8
   scalar solutions in the step -- it does strictly more (hint lookup, the
   walk, the same interpolation).
b. default step unchanged (--baseline-lib PATH, the parent commit's
   libpmx_transfer.so): the plain PMX_RUN_FRESH_BACKGROUND step of both
   builds on each configuration's input, interleaved, two contexts of each
   created alternately; the step total and the surface path's time.
c. end to end -- 16 extra fields through interp_more, host arrays in and
   out, against two extra full steps carrying 8 of them each (upload of the
   background with those fields, step, download): the only way before.

One JSON file (--out, default profiles/many_fields_bench.json).

  python tools/bench_many_fields.py [--configs C3,C2] [--steps 20] [--warmup 3]
                                    [--e2e-reps 3] [--baseline-lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from bench_pointmap import fold, summary, transfer_on  # noqa: E402

KERNELS = ["hint", "vol", "bdy", "exhaustive", "total", "derive"]
# per located point and batch of 8 scalars, bytes that must move
BATCH_BYTES_PER_POINT = 4 + 24 + 1 + 4 + 4 + 32 + 4 * 24 + 4 * 64 + 64 + 1


def scalar_fields(m, k: int, seed: int) -> list[np.ndarray]:
    """k smooth scalar fields on the vertices ((np+1, 1), Mmg layout)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        a, b = rng.uniform(0.5, 4.0, 3), rng.uniform(0.0, 6.0, 3)
        f = np.zeros((m.np + 1, 1))
        f[1:, 0] = np.sin(m.xyz[1:] * a + b).sum(axis=1)
        out.append(f)
    return out


def wall(f) -> float:
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_fields_bench.json"))
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()

    def phase(msg):
        print(f"[bench_many_fields {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    import bench
    from parmmg_amd import _native as N
    from parmmg_amd.transfer import Transfer
    FRESH = N.RUN_FRESH_BACKGROUND
    res = {"steps": args.steps, "warmup": args.warmup, "batch_bytes_per_point": BATCH_BYTES_PER_POINT, "cases": []}
    tr = Transfer(0)
    res["device"] = tr.device_info()
    for cname in args.configs.split(","):
        cfg = bench.CONFIGS[cname]
        phase(f"build_case {cname}")
        m, x, t, sols, tv = bench.build_case(cfg, 0)
        extra = scalar_fields(m, 16, 77)
        # the step: the metric + 4 fields (the configuration's own, then scalars)
        step = (sols + scalar_fields(m, 5, 78))[:5] if sols[0].shape[1] == 1 else ([sols[0]] + scalar_fields(m, 4, 78))
        case = {"config": cname, "ne": m.ne, "np": m.np, "new_points": len(x),
                "step_sizes": [s.shape[1] for s in step]}
        outs = {k: [np.zeros((len(x), 1)) for _ in range(k)] for k in (8, 16)}

        def more(k):
            views_old = (N.SolView * k)()
            views_new = (N.SolView * k)()
            for i in range(k):
                views_old[i].size, views_old[i].m = 1, extra[i].ctypes.data_as(N.dptr)
                views_new[i].size, views_new[i].m = 1, outs[k][i].ctypes.data_as(N.dptr)
            if not tr.lib.pmx_interp_more(tr.ctx, k, views_old, views_new, len(x)):
                raise RuntimeError(tr.lib.pmx_last_error(tr.ctx).decode())

        # ---- a. the yardstick: 8 scalar solutions in the step ----------------
        phase(f"{cname}: k_walks with 8 scalar solutions")
        tr.upload_background(m, [step[0]] + extra[:7] if step[0].shape[1] == 1 else extra[:8],
                             0 if step[0].shape[1] == 1 else -1)
        tr.upload_points(x, t, tets_mmg=tv)
        for _ in range(args.warmup):
            tr.run(flags=FRESH)
        w8, k8 = [], []
        for _ in range(args.steps):
            tr.timing_reset()
            tr.synchronize()
            w8.append(wall(lambda: (tr.run(timing=True, flags=FRESH), tr.synchronize())))
            k8.append([tr.kernel_ms(i) for i in range(len(KERNELS))])
        case["step_8_scalars"] = fold(w8, k8, KERNELS)
        nloc = tr.locate_stats()
        nvol, nbdy = nloc["nvol"], nloc["nbdy"]
        case["located"] = {"volume": nvol, "surface": nbdy}

        # ---- the step with the metric + 4 fields, then the extras ------------
        phase(f"{cname}: step (metric + 4 fields) + 8 / 16 extra scalars")
        tr.upload_background(m, step, 0)
        tr.upload_points(x, t, tets_mmg=tv)
        for _ in range(args.warmup):
            tr.run(flags=FRESH)
            more(8)
            more(16)
        ws, ks = [], []
        wm = {8: [], 16: []}
        km = {8: [], 16: []}
        for _ in range(args.steps):
            tr.timing_reset()
            tr.synchronize()
            ws.append(wall(lambda: (tr.run(timing=True, flags=FRESH), tr.synchronize())))
            ks.append([tr.kernel_ms(i) for i in range(len(KERNELS))])
            for k in (8, 16):
                wm[k].append(wall(lambda: more(k)))
                km[k].append(tr.kernel_ms(7) / (k // 8))
        case["step"] = fold(ws, ks, KERNELS)
        bytes_batch = (nvol + nbdy) * BATCH_BYTES_PER_POINT
        for k in (8, 16):
            kb = summary(km[k])
            case[f"more_{k}"] = {"wall_ms": summary(wm[k]), "kernel_ms_per_batch": kb,
                                 "batch_bytes": bytes_batch,
                                 "batch_GBs": bytes_batch / (kb["median"] * 1e-3) / 1e9}
        yard = case["step_8_scalars"]["vol_ms"]["median"]
        case["batch_over_k_walks"] = case["more_8"]["kernel_ms_per_batch"]["median"] / yard
        phase(f"{cname}: batch {case['more_8']['kernel_ms_per_batch']['median']:.4f} ms "
              f"({case['more_8']['batch_GBs']:.0f} GB/s of {bytes_batch / 1e6:.0f} MB), "
              f"k_walks with 8 scalars {yard:.4f} ms")

        # ---- c. end to end: interp_more vs two extra full steps ---------------
        phase(f"{cname}: end to end, 16 extra fields")
        e_more, e_steps = [], []
        for _ in range(args.e2e_reps):
            tr.upload_background(m, step, 0)
            tr.upload_points(x, t, tets_mmg=tv)
            tr.run(flags=FRESH)
            tr.download(sols_only=True)
            e_more.append(wall(lambda: more(16)))

            def two_steps():
                for h in (0, 1):
                    tr.upload_background(m, extra[8 * h: 8 * h + 8], -1)
                    tr.run(flags=FRESH)
                    tr.download(sols_only=True)
            e_steps.append(wall(two_steps))
        case["end_to_end_16"] = {"interp_more_ms": summary(e_more), "two_full_steps_ms": summary(e_steps),
                                 "ratio": summary(e_steps)["median"] / summary(e_more)["median"]}
        phase(f"{cname}: interp_more {summary(e_more)['median']:.0f} ms, two full steps "
              f"{summary(e_steps)['median']:.0f} ms")
        res["cases"].append(case)

        # ---- b. the default step against the parent build ----------------------
        if args.baseline_lib:
            phase(f"baseline library A/B (plain {cname} step)")
            # two contexts of each build, created alternately (a context's
            # buffers land where the allocator puts them, and the step's time
            # follows: tools/bench_pointmap.py) -- the second pair is the control
            ctxs = []
            for name in ("baseline_a", "this_a", "this_b", "baseline_b"):
                T = transfer_on(args.baseline_lib, 0) if name.startswith("baseline") else Transfer(0)
                T.upload_background(m, sols, 0)
                T.upload_points(x, t, tets_mmg=tv)
                ctxs.append((name, T))
            for _ in range(args.warmup):
                for _, T in ctxs:
                    T.run(flags=FRESH)
            wa = {name: [] for name, _ in ctxs}
            ka = {name: [] for name, _ in ctxs}
            for _ in range(args.steps):
                for name, T in ctxs:
                    T.timing_reset()
                    T.synchronize()
                    wa[name].append(wall(lambda: (T.run(timing=True, flags=FRESH), T.synchronize())))
                    ka[name].append([T.kernel_ms(i) for i in range(len(KERNELS))])
            ab = {name: fold(wa[name], ka[name], KERNELS) for name in wa}
            for lib in ("baseline", "this"):
                for i, kn in ((4, "total"), (2, "bdy")):
                    ab[f"{lib}_{kn}_ms"] = summary([k[i] for n in ("_a", "_b") for k in ka[lib + n]])
            ab["this_minus_baseline_total_ms"] = ab["this_total_ms"]["median"] - ab["baseline_total_ms"]["median"]
            ab["baseline_spread_total_ms"] = ab["baseline_total_ms"]["max"] - ab["baseline_total_ms"]["min"]
            ab["this_minus_baseline_bdy_ms"] = ab["this_bdy_ms"]["median"] - ab["baseline_bdy_ms"]["median"]
            res.setdefault("plain_vs_baseline", {})[cname] = ab
            for kn in ("total_ms", "bdy_ms"):
                phase(f"A/B {kn}, median [min, max]: " + ", ".join(
                    f"{name} {ab[name][kn]['median']:.4f} [{ab[name][kn]['min']:.4f}, "
                    f"{ab[name][kn]['max']:.4f}]" for name in wa))
            for _, T in ctxs:
                T.close()
        del m, x, t, sols, tv, extra, step, outs
    tr.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"out": args.out, "cases": [
        {"config": c["config"], "batch_ms": c["more_8"]["kernel_ms_per_batch"]["median"],
         "k_walks_8_scalars_ms": c["step_8_scalars"]["vol_ms"]["median"],
         "end_to_end_ratio": c["end_to_end_16"]["ratio"]} for c in res["cases"]]}))


if __name__ == "__main__":
    main()
