#!/usr/bin/env python3
"""pmx_metis_graph (PMMG_graph_meshElts2metis, reference src/metis_pmmg.c:
746-823) on the bench's Kuhn cubes: C2 (n = 119) and C3 (n = 255) with the
iso metric h = (0.5 + 2 x) / n, C2 with a rotated tensor metric.

  python tools/bench_metis_graph.py [--cases c2_iso,c3_iso,c2_ani] [--reps 7]
                                    [--twin] [--out profiles/metis_graph_bench.json]

Per case, after 2 warm-up calls, `reps` calls with weights and `reps` without:
the device time of the count, the scan and the fill (HIP events,
pmx_kernel_ms 9 / 10 / 11), the end-to-end host time of the call (it ends in
a stream synchronise: readback of nadjncy, the kernels, the copies of xadj /
adjncy / adjwgt into the caller's preallocated, touched arrays) and, timed
apart, those three copies' bytes over a plain device-to-host copy.  Median,
minimum and maximum of each.

The fill kernel against two yardsticks, the larger of which bounds it:
 (a) its compulsory bytes -- reads 32 ne + np (24 + 8 msize), writes
     4 (ne + 1) + 8 nadjncy -- over the measured streaming ceiling of the
     device (6.29 TB/s, a float4 copy);
 (b) 6 ne edge lengths at the per-edge time of k_prilen in
     profiles/r06_c5share_stats_iso.json (2.80 ms / 146 259 575 edges).
--twin: the one-core time of the C twin (tests/c/metis_graph_ref.c, glibc,
-O3) on the same input and host, for scale.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_BPS = 6.29e12
CASES = {"c2_iso": (119, "iso"), "c3_iso": (255, "iso"), "c2_ani": (119, "ani"),
         "tiny_iso": (12, "iso"), "tiny_ani": (12, "ani")}


def prilen_edge_seconds():
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_c5share_stats_iso.json")))["prilen"]
    return d["ms"] * 1e-3 / (d["ned"] + d.get("nullEdge", 0))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def run_case(name, reps, twin):
    import numpy as np
    import metis_ref as R
    from parmmg_amd import _native as N
    from parmmg_amd import mesh as M
    from parmmg_amd.transfer import Transfer

    n, kind = CASES[name]
    t0 = time.perf_counter()
    m = M.kuhn_cube(n)
    met = R.iso_sizes(m, n) if kind == "iso" else R.rotated_tensor(m, n)
    tr = Transfer(0)
    tr.upload_background(m, [met], 0)
    setup_s = time.perf_counter() - t0
    ne, msize = m.ne, met.shape[1]
    xadj = np.zeros(ne + 1, np.int32)
    adjncy = np.zeros(4 * ne, np.int32)
    adjwgt = np.zeros(4 * ne, np.int32)
    cnt = C.c_int64()
    p = lambda a: a.ctypes.data_as(N.i32ptr)

    def call(weights):
        t = time.perf_counter()
        r = tr.lib.pmx_metis_graph(tr.ctx, 0, p(xadj), p(adjncy), p(adjwgt) if weights else None, len(adjncy),
                                   C.byref(cnt))
        dt = time.perf_counter() - t
        if not r:
            raise RuntimeError(tr.lib.pmx_last_error(tr.ctx).decode())
        return dt * 1e3, [tr.kernel_ms(w) for w in (9, 10, 11)]

    out = {"n": n, "metric": kind, "ne": ne, "np": m.np, "msize": msize, "setup_s": setup_s}
    for weights in (True, False):
        for _ in range(2):
            call(weights)
        e2e, ks = [], []
        for _ in range(reps):
            a, b = call(weights)
            e2e.append(a)
            ks.append(b)
        key = "weights" if weights else "no_weights"
        out[key] = {"end_to_end_ms": spread(e2e), "count_ms": spread([k[0] for k in ks]),
                    "scan_ms": spread([k[1] for k in ks]), "fill_ms": spread([k[2] for k in ks]),
                    "outside_kernels_ms": spread([a - sum(k) for a, k in zip(e2e, ks)])}
    nadj = cnt.value
    out["nadjncy"] = nadj
    out["int_weights"] = {"min": int(adjwgt[:nadj].min()), "max": int(adjwgt[:nadj].max()),
                          "clamped_frac": float((adjwgt[:nadj] == 1000000).mean())}
    # the three arrays' bytes as one plain device-to-host copy into touched memory
    nbytes = 4 * (ne + 1) + 8 * nadj
    dev = tr.lib.pmx_device_alloc(tr.ctx, nbytes)
    if dev:
        host = np.zeros(nbytes, np.uint8)
        dl = []
        for i in range(reps + 1):
            t = time.perf_counter()
            tr.lib.pmx_device_download(tr.ctx, host.ctypes.data_as(C.c_void_p), C.c_void_p(dev), nbytes)
            if i:
                dl.append((time.perf_counter() - t) * 1e3)
        tr.lib.pmx_device_free(tr.ctx, C.c_void_p(dev))
        out["download"] = {"bytes": nbytes, "ms": spread(dl), "GBs": nbytes / statistics.median(dl) / 1e6}
    rd = 32 * ne + m.np * (24 + 8 * msize)
    wr = 4 * (ne + 1) + 8 * nadj
    fill = out["weights"]["fill_ms"]["median"] * 1e-3
    ya = (rd + wr) / STREAM_BPS
    yb = 6 * ne * prilen_edge_seconds()
    out["fill_yardsticks"] = {
        "read_bytes": rd, "write_bytes": wr, "a_bytes_ms": ya * 1e3, "b_lengths_ms": yb * 1e3,
        "larger": "a (bytes at the streaming ceiling)" if ya >= yb else "b (edge lengths at k_prilen's cost)",
        "fill_ms": fill * 1e3, "fill_over_a": fill / ya, "fill_over_b": fill / yb,
        "fill_GBs": (rd + wr) / fill / 1e9,
        "fill_edge_ps": fill / (6 * ne) * 1e12, "prilen_edge_ps": prilen_edge_seconds() * 1e12}
    # without weights the fill reads the records and xadj and writes adjncy: bytes only
    nb = 32 * ne + 4 * (ne + 1) + 4 * nadj
    f0 = out["no_weights"]["fill_ms"]["median"] * 1e-3
    out["fill_no_weights"] = {"bytes": nb, "bytes_ms": nb / STREAM_BPS * 1e3, "fill_ms": f0 * 1e3,
                              "GBs": nb / f0 / 1e9, "frac_of_ceiling": nb / f0 / STREAM_BPS}
    if twin:
        t = time.perf_counter()
        g = R.graph(m, met, lengths=False)
        out["twin_one_core_s"] = time.perf_counter() - t
        d = adjwgt[:nadj].astype(np.int64) - g["iwgt"]
        out["twin_check"] = {"adjncy_equal": bool(np.array_equal(adjncy[:nadj], g["adjncy"])),
                             "weights_differing": int((d != 0).sum()), "max_abs_diff": int(np.abs(d).max())}
    tr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2_iso,c3_iso,c2_ani")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from parmmg_amd import build
    build.build_meshgen()
    build.build_transfer()
    res = {"tool": "tools/bench_metis_graph.py", "reps": args.reps, "stream_ceiling_Bps": STREAM_BPS, "cases": {}}
    for name in args.cases.split(","):
        res["cases"][name] = run_case(name, args.reps, args.twin)
        print(json.dumps({name: res["cases"][name]}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
