#!/usr/bin/env python
"""quadrature on the device: one JSON line per case.

  ms_per_call   wall time of one lsm_quad_create (classify sweep, compaction, count pass, scans, emit pass and the two
                host reads of the counts), median of --reps calls after one warm-up call
  ncut, nfull   cut cells with nodes, full cells (volume: every coefficient < 0)
  nodes         nodes of the cut cells; nodes_per_s = nodes / ms_per_call
  total, exact  the sum of the weights (lsm_quad_total) against 4πR² / 4πR³/3 (sphere) or 2πR / πR² (disk)
Cases: the exact-distance sphere ‖x‖ - 0.5 in [-1, 1]³ at 128³, 256³ and 512³, and the disk in [-1, 1]² at 4096², each
surface and volume, interpolation_order 3, quadrature_order 4.
--trace writes the kernel statistics of a rocprofv3 --kernel-trace --stats directory as JSON (the classify sweep's
fraction of HBM peak under its traffic model: the field read once and one class byte written per cell)."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import lsm_amd as lsm

HBM_PEAK = 8.0e12
CASES = {"sphere128": (3, 128), "sphere256": (3, 256), "sphere512": (3, 512), "disk4096": (2, 4096)}


def field(N, n):
    grid = lsm.CartesianGrid((-1.0,) * N, (1.0,) * N, (n,) * N)
    ax = np.linspace(-1.0, 1.0, n)
    if N == 2:
        vals = np.hypot(ax[:, None], ax[None, :]) - 0.5
    else:
        vals = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5
    mf = lsm.MeshField(np.asfortranarray(vals), grid)
    del vals
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.ExtrapolationBC(3)).current_state()


def run(name, reps):
    N, n = CASES[name]
    phi = field(N, n)
    b = phi.backend
    b.fill_ghosts(phi.buf)
    for surface in (True, False):
        h, counts = b.quad_create(phi.buf, None, 3, 4, surface)
        b.quad_destroy(h)
        ts = []
        for _ in range(reps):
            b.sync()
            t = time.perf_counter()
            h, counts = b.quad_create(phi.buf, None, 3, 4, surface)
            ts.append((time.perf_counter() - t) * 1e3)
            if _ < reps - 1:
                b.quad_destroy(h)
        total = b.quad_total(h)
        b.quad_destroy(h)
        R = 0.5
        exact = (4 * math.pi * R ** 2 if surface else 4 / 3 * math.pi * R ** 3) if N == 3 else (2 * math.pi * R if surface else math.pi * R ** 2)
        ms = statistics.median(ts)
        ncut, nodes, nfull, nfb = counts
        print(json.dumps({"case": name, "n": n, "ndim": N, "surface": surface, "interpolation_order": 3, "quadrature_order": 4, "reps": reps,
                          "ms_per_call": round(ms, 3), "ncut": ncut, "nfull": nfull, "nodes": nodes, "nfallback": nfb,
                          "nodes_per_s": round(nodes / (ms * 1e-3)), "total": total, "exact": exact,
                          "rel_err": abs(total - exact) / exact}), flush=True)


def trace(dirname, name):
    """kernel statistics of a rocprofv3 run of `--cases name`"""
    f = glob.glob(dirname + "/**/*kernel_stats.csv", recursive=True)[0]
    N, n = CASES[name]
    ncell = (n - 1) ** N
    out = {}
    for r in csv.DictReader(open(f)):
        kname = r["Name"].split("(")[0]
        if "quad" not in kname and "chunk_scan_kernel" not in kname:      # chunk_scan: the shared scan (csrc/scan.h)
            continue
        e = out.setdefault(kname.replace("void ", ""), {"dispatches": 0, "total_ms": 0.0})
        e["dispatches"] += int(r["Calls"])
        e["total_ms"] += int(r["TotalDurationNs"]) / 1e6
    for k, e in out.items():
        e["total_ms"] = round(e["total_ms"], 3)
        e["us_per_dispatch"] = round(1e3 * e["total_ms"] / e["dispatches"], 1)
        if "classify" in k:
            bpc = 8 + 1          # the field read once (fp64), one class byte written
            e["model_bytes_per_cell"] = bpc
            e["model_gbs"] = round(bpc * ncell / (e["total_ms"] / e["dispatches"] * 1e-3) / 1e9, 1)
            e["hbm_frac"] = round(e["model_gbs"] * 1e9 / HBM_PEAK, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", help="a rocprofv3 output directory: print its quadrature kernel statistics as JSON")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(trace(a.trace, a.cases.split(",")[0]), indent=1))
        return
    for name in a.cases.split(","):
        run(name, a.reps)


if __name__ == "__main__":
    main()
