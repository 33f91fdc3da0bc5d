#!/usr/bin/env python
"""mesh_distance on the device: writes profiles/mesh_distance/mdist_bench.json (and prints one JSON line per case).

The workload: the isosurface mesh of the exact-distance sphere ‖x‖ − 0.5 in [−1, 1]³ at 256³ (extracted on the device, never
leaving it) measured back onto its own grid with the cutoff c = 4h.
  ms_per_call    wall time of one lsm_mesh_distance (validation kernel and its host read, the memsets, the distance, sign and
                 final passes, the host read of the statistics), median of --reps calls after one warm-up call
  pairs          element–node pairs the distance pass visits: Σ over the elements of the nodes in the bounding box dilated by c
                 and clipped to the grid (the cost model of DESIGN.md §7.14), counted on the host from the mesh
  pairs_per_s    pairs / ms_per_call
and on the 64³ sphere the same call with c = 4h and with c = inf (every element against every node): what the cutoff saves.
`empty_ms`: the call with an empty mesh — memsets, the init kernel, the final pass, one synchronise — an upper bound of the final
pass's time; its rate under the traffic model (the final pass reads 8 + 4 and writes 8 bytes per node) as a fraction of
`--copy-tbs`, what tools/copy_bw reaches on the same box with 8 bytes per lane (read + write; the tool is run when the option is
absent and the program is built).

Kernel times: run the same command with --no-write under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, then
`--stats DIR` adds every md_* kernel's dispatches and total time and the final pass's own rate (run the traced command with
--flagship-only: every dispatch is then the 256³ grid's)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

OUT = os.path.join(ROOT, "profiles", "mesh_distance")
MARGIN = 1.0 / 1024       # csrc/lsm_mdist.hip, MD_MARGIN
FINAL_BYTES_PER_NODE = 20


def field(lsm, n):
    grid = lsm.CartesianGrid((-1.0,) * 3, (1.0,) * 3, (n,) * 3)
    ax = np.linspace(-1.0, 1.0, n)
    vals = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.asfortranarray(vals), grid), bc=lsm.NeumannBC()).current_state()


def count_pairs(verts, elems, n, c):
    """Σ of the dilated, clipped bounding boxes, as md_box counts them"""
    p = verts[elems]
    h = 2.0 / (n - 1)
    tlo = (p.min(axis=1) - c + 1.0) / h - MARGIN
    thi = (p.max(axis=1) + c + 1.0) / h + MARGIN
    lo = np.clip(np.ceil(tlo), 0, n)
    hi = np.clip(np.floor(thi), -1, n - 1)
    return int(np.prod(np.maximum(hi - lo + 1, 0), axis=1).sum())


def timed(b, reps, call):
    call()
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def run(lsm, n, cutoffs, reps):
    src = field(lsm, n)
    b = src.backend
    h_iso, counts = b.iso_create(src.buf, None, 0.0)
    verts, elems = b.iso_read(h_iso, counts)
    b.iso_destroy(h_iso)
    hv, he = verts.cpu().numpy(), elems.cpu().numpy()
    phi = src.copy()
    h = 2.0 / (n - 1)
    out = []
    for cells in cutoffs:
        c = float("inf") if cells is None else cells * h
        stats = []
        ms, lo, hi = timed(b, reps, lambda: stats.append(b.mesh_distance(phi.buf, verts, elems, c)))
        pairs = count_pairs(hv, he, n, c) if cells is not None else len(he) * n ** 3
        res = {"case": f"sphere{n}", "n": n, "cutoff_cells": cells, "reps": reps, "vertices": len(hv), "elements": len(he),
               "ms_per_call": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "pairs": pairs,
               "pairs_per_s": round(pairs / (ms * 1e-3)), "near_nodes": stats[-1][0], "unbalanced_rows": stats[-1][1],
               "skipped_elements": stats[-1][2]}
        print(json.dumps(res), flush=True)
        out.append(res)
    empty_v, empty_e = verts[:0], elems[:0]
    ms, lo, hi = timed(b, reps, lambda: b.mesh_distance(phi.buf, empty_v, empty_e, 4 * h))
    empty = {"case": f"sphere{n}", "n": n, "empty_ms": round(ms, 3), "empty_ms_min": round(lo, 3),
             "empty_model_gbs": round(FINAL_BYTES_PER_NODE * n ** 3 / (ms * 1e-3) / 1e9, 1)}
    print(json.dumps(empty), flush=True)
    return out, empty


def copy_yardstick():
    """TB/s (read + write) of tools/copy_bw's 8-bytes-per-lane copy, one element per thread"""
    exe = os.path.join(ROOT, "tools", "copy_bw")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"8 B/lane, one element per thread\s+[\d.]+ ms\s+([\d.]+) TB/s", out)
    return float(m.group(1)) if m else None


def kernel_stats(dirname):
    f = glob.glob(dirname + "/**/*kernel_stats.csv", recursive=True)[0]
    out = {}
    for r in csv.DictReader(open(f)):
        kname = r["Name"].split("(")[0].replace("void ", "")
        if "::md_" not in kname:
            continue
        e = out.setdefault(kname, {"dispatches": 0, "total_ms": 0.0})
        e["dispatches"] += int(r["Calls"])
        e["total_ms"] += int(r["TotalDurationNs"]) / 1e6
    for e in out.values():
        e["total_ms"] = round(e["total_ms"], 3)
        e["us_per_dispatch"] = round(1e3 * e["total_ms"] / e["dispatches"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256, help="the flagship grid (default 256)")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the md_* kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/mesh_distance)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    ap.add_argument("--flagship-only", action="store_true", help="skip the 64^3 cases (the run under the profiler: every dispatch is the flagship grid's)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "mdist_bench.json")
    if a.stats:
        doc = json.load(open(path))
        ks = kernel_stats(a.stats)
        doc["kernel_trace"] = {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/mdist_bench.py --no-write --flagship-only; "
                                      "python tools/mdist_bench.py --stats <dir>",
                               "note": "the flagship grid's calls, warm-up and empty-mesh calls included (traced, so slower than the plain run)", "kernels": ks}
        fin = [v for k, v in ks.items() if "md_final_kernel" in k]
        if fin:
            gbs = FINAL_BYTES_PER_NODE * doc["cases"][0]["n"] ** 3 / (fin[0]["us_per_dispatch"] * 1e-6) / 1e9
            doc["kernel_trace"]["final_model_gbs"] = round(gbs, 1)
            if doc.get("copy_tbs_8B_per_lane"):
                doc["kernel_trace"]["final_frac_of_copy"] = round(gbs / (doc["copy_tbs_8B_per_lane"] * 1e3), 3)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    flagship, empty = run(lsm, a.n, [4], a.reps)
    if a.no_write or a.flagship_only:
        return
    small, _ = run(lsm, 64, [4, None], a.reps)
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        empty["empty_frac_of_copy"] = round(empty["empty_model_gbs"] / (copy_tbs * 1e3), 3)
    saved = {"pairs_cutoff_4h": small[0]["pairs"], "pairs_no_cutoff": small[1]["pairs"],
             "pairs_saved_fraction": round(1 - small[0]["pairs"] / small[1]["pairs"], 5),
             "ms_cutoff_4h": small[0]["ms_per_call"], "ms_no_cutoff": small[1]["ms_per_call"]}
    doc = {"cmd": "python tools/mdist_bench.py --reps %d" % a.reps, "device": "MI355X (gfx950), 1 GPU", "copy_tbs_8B_per_lane": copy_tbs,
           "final_model_bytes_per_node": FINAL_BYTES_PER_NODE, "cases": flagship + small, "final_pass_upper_bound": empty, "cutoff_64": saved}
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
