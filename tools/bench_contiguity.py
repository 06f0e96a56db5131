#!/usr/bin/env python3
"""pmx_contiguity / pmx_fix_contiguity (PMMG_check_part_contiguity and
PMMG_fix_contiguity_split, reference src/metis_pmmg.c:312-392 and
src/moveinterfaces_pmmg.c:377-449) on the bench's Kuhn cubes: C2 (n = 119) and
C3 (n = 255).

  python tools/bench_contiguity.py [--cases c2,c3] [--reps 5] [--twin]
                                   [--sweep-limit 120] [--out profiles/contiguity_bench.json]

Per case, on a partition into 8 z-slabs:
 (a) the labelling (Transfer.contiguity with counts and labels): device time
     (HIP events, pmx_kernel_ms 12) and the wall time of the call, which
     includes the upload of part[] and the download of the labels;
 (b) the fix of that partition with 1,000 planted fragments (500 single tets,
     500 tets with their face neighbours): labelling and replay + recolour
     device time (pmx_kernel_ms 12 / 13), wall time including both copies of
     part[], and the rounds, relabels, replay launches and dequeues.
The stored quality call (pmx_tetra_qual, an existing path) is timed before and
after, spread reported, no threshold.

Labelling bytes (algorithmic): per hooking round 32 B of tet record + 4 B of
mark + 4 B of parent per tet, and the pointer jump's 4 B read + 4 B write; the
size pass reads 32 + 4 B per tet, the table pass 4 B.  The achieved fraction is
these bytes over the device time over the streaming ceiling (6.29 TB/s, a
float4 copy); the gathers of the neighbours' marks and parents come on top and
are not counted.

--twin: the one-core C twin (tests/c/contiguity_ref.c) on the same input,
asserted equal.  The reference's sweep counters are timed at C2 only, in a
child process that is stopped after --sweep-limit seconds ("> N s").
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_BPS = 6.29e12
CASES = {"c2": 119, "c3": 255, "tiny": 12}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def partition(m, n_frag=1000, seed=3):
    """(8 z-slabs, the same with n_frag fragments planted)."""
    import numpy as np
    import contiguity_ref as R
    clean = R.slabs(m, 8)
    part = clean.copy()
    rng = np.random.default_rng(seed)
    seeds = rng.choice(m.ne, n_frag, replace=False)
    colour = (clean[seeds] + 3) % 8
    part[seeds] = colour
    blob = seeds[n_frag // 2:]
    nb = m.adja[1:4 * m.ne + 1].reshape(m.ne, 4)[blob] // 4
    for f in range(4):
        ok = nb[:, f] > 0
        part[nb[ok, f] - 1] = colour[n_frag // 2:][ok]
    return clean, part


def sweep_child(n):
    import contiguity_ref as R
    from parmmg_amd import mesh as M
    m = M.kuhn_cube(n)
    t = time.perf_counter()
    g = R.sweep_group(m)
    t_group = time.perf_counter() - t
    t = time.perf_counter()
    last, counts = R.sweep_parts(m, R.slabs(m, 8), 8)
    print(json.dumps({"group_s": t_group, "group_count": g, "parts_s": time.perf_counter() - t,
                      "parts_counts": [int(c) for c in counts]}))


def run_case(name, reps, twin, sweep_limit):
    import numpy as np
    import contiguity_ref as R
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer

    n = CASES[name]
    m = M.kuhn_cube(n)
    ne = m.ne
    clean, planted = partition(m)
    tr = Transfer(0)
    tr.upload_background(m, [np.ones((m.np + 1, 1))], 0)
    out = {"n": n, "ne": ne}

    def qual():
        ts = []
        for i in range(reps + 1):
            t = time.perf_counter()
            tr.tetra_qual(ne)
            if i:
                ts.append((time.perf_counter() - t) * 1e3)
        return spread(ts)

    out["tetra_qual_before_ms"] = qual()
    # (a) labelling
    wall, dev = [], []
    for i in range(reps + 1):
        t = time.perf_counter()
        ncomp, counts, label = tr.contiguity(clean, 8)
        if i:
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(tr.kernel_ms(12))
    _, st_clean = tr.fix_contiguity(clean, 8)
    rounds = st_clean["rounds"]
    nbytes = rounds * ne * (32 + 4 + 4 + 8) + ne * (32 + 4) + ne * 4
    d = statistics.median(dev) * 1e-3
    out["label"] = {"ncomp": ncomp, "counts": [int(c) for c in counts], "rounds": rounds, "wall_ms": spread(wall),
                    "device_ms": spread(dev), "algorithmic_bytes": nbytes, "GBs": nbytes / d / 1e9,
                    "frac_of_ceiling": nbytes / d / STREAM_BPS}
    # (b) fix with planted fragments
    wall, lab, rep = [], [], []
    for i in range(reps + 1):
        t = time.perf_counter()
        fixed, st = tr.fix_contiguity(planted, 8)
        if i:
            wall.append((time.perf_counter() - t) * 1e3)
            lab.append(tr.kernel_ms(12))
            rep.append(tr.kernel_ms(13))
    out["fix"] = {"stats": st, "wall_ms": spread(wall), "label_device_ms": spread(lab),
                  "replay_device_ms": spread(rep), "changed_tets": int((fixed != planted).sum()),
                  "clean_again": bool(np.array_equal(fixed, clean))}
    _, st3 = tr.fix_contiguity(planted, 8, 64)
    out["fix_replay_steps_64"] = st3
    out["tetra_qual_after_ms"] = qual()
    tr.close()
    if twin:
        t = time.perf_counter()
        n_t, c_t, l_t = R.components(m, clean, 8)
        out["twin_components_s"] = time.perf_counter() - t
        assert n_t == ncomp and np.array_equal(c_t, counts) and np.array_equal(l_t, label)
        t = time.perf_counter()
        f_t, s_t = R.fix(m, planted, 8)
        out["twin_fix_s"] = time.perf_counter() - t       # includes its own component count
        assert np.array_equal(f_t, fixed) and all(st[k] == v for k, v in s_t.items())
        out["twin_equal"] = True
        if name == "c2" or name == "tiny":
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-child", str(n)],
                                   capture_output=True, text=True, timeout=sweep_limit)
                out["reference_sweeps"] = json.loads(r.stdout.strip().splitlines()[-1])
            except subprocess.TimeoutExpired:
                out["reference_sweeps"] = f"> {sweep_limit} s"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--sweep-limit", type=int, default=120)
    ap.add_argument("--sweep-child", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from parmmg_amd import build
    build.build_meshgen()
    if args.sweep_child:
        sweep_child(args.sweep_child)
        return
    build.build_transfer()
    res = {"tool": "tools/bench_contiguity.py", "reps": args.reps, "stream_ceiling_Bps": STREAM_BPS, "cases": {}}
    for name in args.cases.split(","):
        res["cases"][name] = run_case(name, args.reps, args.twin, args.sweep_limit)
        print(json.dumps({name: res["cases"][name]}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
