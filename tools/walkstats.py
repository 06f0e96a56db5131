#!/usr/bin/env python3
"""Walk diagnostics on a bench config (GPU): histogram of walk steps, distance
from the hint start, ties / stuck counts.

  python tools/walkstats.py --config C2 [--flags F] [--hint-stride S]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--hint-stride", type=int, default=0)
    args = ap.parse_args()
    import bench
    from parmmg_amd import build
    build.build_meshgen()
    build.build_transfer()
    from parmmg_amd.transfer import Transfer
    cfg = bench.CONFIGS[args.config]
    m, x, t, sols, _ = bench.build_case(cfg, 0)
    tr = Transfer(0)
    tr.upload_background(m, sols, 0)
    tr.upload_points(x, t)
    tr.run(flags=args.flags, hint_stride=args.hint_stride, record_starts=True)
    r = tr.download()
    st = tr.starts()
    vol = t == 0
    steps = r.steps[vol]
    h = np.bincount(np.clip(np.abs(steps), 0, 20))
    c = m.centroids()
    d = np.linalg.norm(c[st[vol] - 1] - x[vol], axis=1) * cfg["n"]
    # the grid the step built, held to the definitions of tests/start_ref.py
    # with the descriptor the kernels used (any box, any dims)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import start_ref
    desc, cells = tr.debug_grid(0)
    order = 2 if os.environ.get("PMX_HINT_SAMPLE_ORDER") == "2" else 0
    bad = start_ref.check_sizing(m, desc, cells.size, 0) + start_ref.check_volume_cells(m, desc, cells,
                                                                                        args.hint_stride, order)
    gi = cells.ravel().astype(np.int64)
    nz = np.nonzero(gi > 0)[0]
    ks = start_ref.sample(m, args.hint_stride, order)
    home = np.full(m.ne + 2, -1, np.int64)
    home[ks] = start_ref.cell_of(m, desc, ks)
    wrong = int((home[np.minimum(gi[nz], m.ne + 1)] != nz).sum())
    out_grid = {"dim": [int(v) for v in desc["dim"]], "cells": int(cells.size), "empty": int(cells.size - len(nz)),
                "wrong_cell": wrong, "violations": bad}
    out = {"grid": out_grid, "config": args.config, "n": cfg["n"], "nvol": int(vol.sum()),
           "steps_hist": {int(i): int(v) for i, v in enumerate(h) if v},
           "steps_mean": float(np.abs(steps).mean()),
           "start_dist_cells": {"mean": float(d.mean()), "p50": float(np.median(d)),
                                "p99": float(np.percentile(d, 99)), "max": float(d.max())},
           "status": {int(k): int(v) for k, v in zip(*np.unique(r.status[vol], return_counts=True))},
           "stats": tr.locate_stats()}
    # surface path: steps per point and per wave (64 consecutive list entries)
    bdy = np.nonzero(t == 16)[0]
    if len(bdy):
        bs = np.abs(r.steps[bdy]).astype(np.int64)
        pad = (-len(bs)) % 64
        wmax = np.concatenate([bs, np.zeros(pad, np.int64)]).reshape(-1, 64).max(1)
        out["bdy"] = {"n": int(len(bdy)), "steps_mean": float(bs.mean()),
                      "steps_hist": {int(i): int(v) for i, v in enumerate(np.bincount(np.clip(bs, 0, 40))) if v},
                      "wave_max_mean": float(wmax.mean()), "wave_max_max": int(wmax.max()),
                      "status": {int(k): int(v) for k, v in zip(*np.unique(r.status[bdy], return_counts=True))}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
