#!/usr/bin/env python
"""volume_mesh on the device: writes profiles/volume_mesh/vol_bench.json (and prints one JSON line per case).

  ms_per_call    wall time of one lsm_vol_create (classify sweep, scan, the host read of the counts, offsets, vertex and element
                 kernels, the final synchronise), median of --reps calls after one warm-up call
  vertices, elements, interface_elements, elements_per_s = elements / ms_per_call
Cases: the exact-distance sphere ‖x‖ − 0.5 in [−1, 1]³ at 128³, 256³ and 512³ and the disk in [−1, 1]² at 4096².

The element kernel's rate needs kernel times: run the same command under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vol_bench.py --no-write` (a run of its own) and then
`python tools/vol_bench.py --merge --trace DIR`: the kernel's dispatches are taken case by case in order (--reps + 1 each), the
median of the timed ones; its output — (N + 1) int64 per element and N per interface element — per second, and that as a
fraction of `copy_tbs_8B_per_lane`, what tools/copy_bw reaches on the same box in the plain run with 8 bytes per lane, one
element per thread (read + write; the tool is run when --copy-tbs is absent and the program is built).  The kernel statistics of
the traced run go to profiles/volume_mesh/kernel_stats.json."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from iso_bench import copy_yardstick

OUT = os.path.join(ROOT, "profiles", "volume_mesh")
CASES = {"sphere128": (3, 128), "sphere256": (3, 256), "sphere512": (3, 512), "disk4096": (2, 4096)}


def field(lsm, N, n):
    grid = lsm.CartesianGrid((-1.0,) * N, (1.0,) * N, (n,) * N)
    ax = np.linspace(-1.0, 1.0, n)
    if N == 2:
        vals = np.hypot(ax[:, None], ax[None, :]) - 0.5
    else:
        vals = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5
    mf = lsm.MeshField(np.asfortranarray(vals), grid)
    del vals
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def run(lsm, name, reps):
    N, n = CASES[name]
    phi = field(lsm, N, n)
    b = phi.backend
    h, counts = b.vol_create(phi.buf, None, 0.0)
    b.vol_destroy(h)
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        h, counts = b.vol_create(phi.buf, None, 0.0)
        ts.append((time.perf_counter() - t) * 1e3)
        b.vol_destroy(h)
    ms = statistics.median(ts)
    nv, ne, ni = counts
    res = {"case": name, "n": n, "ndim": N, "reps": reps, "ms_per_call": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
           "vertices": nv, "elements": ne, "interface_elements": ni, "elements_per_s": round(ne / (ms * 1e-3)),
           "output_bytes": 8 * (nv * N + ne * (N + 1) + ni * N)}
    print(json.dumps(res), flush=True)
    return res


def element_rates(dirname, cases, reps, copy_tbs):
    """per case: the element kernel's µs (median of the timed dispatches), its output in GB/s, the fraction of the yardstick"""
    f = glob.glob(dirname + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "vol_element_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(cases) * (reps + 1), (len(rows), len(cases), reps)
    out = {}
    for i, c in enumerate(cases):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * (reps + 1) + 1:(i + 1) * (reps + 1)]]
        N = c["ndim"]
        nbytes = 8 * (c["elements"] * (N + 1) + c["interface_elements"] * N)
        gbs = nbytes / (statistics.median(us) * 1e-6) / 1e9
        out[c["case"]] = {"element_kernel_us": round(statistics.median(us), 1), "element_kernel_output_bytes": nbytes,
                          "element_kernel_output_gbs": round(gbs, 1)}
        if copy_tbs:
            out[c["case"]]["element_kernel_frac_of_copy"] = round(gbs / (copy_tbs * 1e3), 3)
    return out


def kernel_stats(dirname):
    f = glob.glob(dirname + "/**/*kernel_stats.csv", recursive=True)[0]
    out = {}
    for r in csv.DictReader(open(f)):
        kname = r["Name"].split("(")[0].replace("void ", "")
        if "vol_" not in kname and "kuhn_" not in kname and "chunk_scan_kernel" not in kname:     # the scan of the chunk sums is shared (csrc/scan.h)
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
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--trace", help="with --merge: the directory of the rocprofv3 --kernel-trace --stats run of the same command")
    ap.add_argument("--merge", action="store_true", help="add the element kernel's rates to the existing vol_bench.json, run nothing")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/volume_mesh)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "vol_bench.json")
    if a.merge:
        doc = json.load(open(path))
        rates = element_rates(a.trace, doc["cases"], doc["cases"][0]["reps"], doc.get("copy_tbs_8B_per_lane"))
        for c in doc["cases"]:
            c.update(rates[c["case"]])
        json.dump(doc, open(path, "w"), indent=1)
        json.dump({"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/vol_bench.py --no-write; "
                          "python tools/vol_bench.py --merge --trace <dir>",
                   "case": "all cases: %d calls of lsm_vol_create each (one warm-up)" % (doc["cases"][0]["reps"] + 1), "kernels": kernel_stats(a.trace)},
                  open(os.path.join(a.out, "kernel_stats.json"), "w"), indent=1)
        return
    import lsm_amd as lsm
    res = [run(lsm, name, a.reps) for name in a.cases.split(",")]
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    json.dump({"cmd": "python tools/vol_bench.py --reps %d" % a.reps, "device": "MI355X (gfx950), 1 GPU", "copy_tbs_8B_per_lane": copy_tbs,
               "cases": res}, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
