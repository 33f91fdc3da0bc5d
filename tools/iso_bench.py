#!/usr/bin/env python
"""isosurface on the device: writes profiles/isosurface/iso_bench.json (and prints one JSON line per case).

  ms_per_call    wall time of one lsm_iso_create (classify sweep, scan, the host read of the counts, compaction, vertex and
                 element kernels, the final synchronise), median of --reps calls after one warm-up call
  vertices, elements, elements_per_s = elements / ms_per_call
Cases: the exact-distance sphere ‖x‖ − 0.5 in [−1, 1]³ at 128³, 256³ and 512³, the disk in [−1, 1]² at 4096², and the
narrow band (nlayers 3, float32 storage) of the sphere at 768³ as in BASELINE config 5.

The classify sweep's rate needs kernel times: run the same command under `rocprofv3 --kernel-trace --output-format csv -d DIR`
and pass `--trace DIR` to the plain run (or `--trace DIR --merge` afterwards): the sweep's dispatches are taken case by case in
order (--reps + 1 each), the median of the timed ones, as GB/s under the traffic model — the field read once (8 or 4 bytes per
node) and two bytes written per node — and as a fraction of `--copy-tbs`, what tools/copy_bw reaches on the same box with 8
bytes per lane, one element per thread (read + write; the tool is run when the option is absent and the program is built).
--stats DIR NAME writes the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of `--cases NAME` next to it."""
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

OUT = os.path.join(ROOT, "profiles", "isosurface")
CASES = {"sphere128": (3, 128, False), "sphere256": (3, 256, False), "sphere512": (3, 512, False), "disk4096": (2, 4096, False),
         "band768": (3, 768, True)}


def field(lsm, N, n, band):
    grid = lsm.CartesianGrid((-1.0,) * N, (1.0,) * N, (n,) * N)
    ax = np.linspace(-1.0, 1.0, n)
    if N == 2:
        vals = np.hypot(ax[:, None], ax[None, :]) - 0.5
    else:
        vals = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5
    if band:
        mf = lsm.NarrowBandMeshField(lsm.MeshField(np.asfortranarray(vals.astype(np.float32)), grid, dtype=np.float32), nlayers=3)
    else:
        mf = lsm.MeshField(np.asfortranarray(vals), grid)
    del vals
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def run(lsm, name, reps):
    N, n, band = CASES[name]
    phi = field(lsm, N, n, band)
    b = phi.backend
    mask = phi.mask if band else None
    h, counts = b.iso_create(phi.buf, mask, 0.0)
    b.iso_destroy(h)
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        h, counts = b.iso_create(phi.buf, mask, 0.0)
        ts.append((time.perf_counter() - t) * 1e3)
        b.iso_destroy(h)
    ms = statistics.median(ts)
    nv, ne = counts
    res = {"case": name, "n": n, "ndim": N, "band": band, "storage": "float32" if band else "float64", "reps": reps,
           "ms_per_call": round(ms, 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "vertices": nv, "elements": ne,
           "elements_per_s": round(ne / (ms * 1e-3))}
    if band:
        res["active_nodes"] = phi.active_count()
    print(json.dumps(res), flush=True)
    return res


def copy_yardstick():
    """TB/s (read + write) of tools/copy_bw's 8-bytes-per-lane copy, one element per thread"""
    exe = os.path.join(ROOT, "tools", "copy_bw")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"8 B/lane, one element per thread\s+[\d.]+ ms\s+([\d.]+) TB/s", out)
    return float(m.group(1)) if m else None


def classify_rates(dirname, cases, reps, copy_tbs):
    """per case: the classify sweep's µs (median of the timed dispatches), GB/s under the traffic model, fraction of the yardstick"""
    f = glob.glob(dirname + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((r for r in csv.DictReader(open(f)) if "iso_classify_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(cases) * (reps + 1), (len(rows), len(cases), reps)
    out = {}
    for i, name in enumerate(cases):
        N, n, band = CASES[name]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * (reps + 1) + 1:(i + 1) * (reps + 1)]]
        bpn = (4 if band else 8) + 2
        gbs = bpn * n ** N / (statistics.median(us) * 1e-6) / 1e9
        out[name] = {"classify_us": round(statistics.median(us), 1), "model_bytes_per_node": bpn, "classify_model_gbs": round(gbs, 1)}
        if copy_tbs:
            out[name]["classify_frac_of_copy"] = round(gbs / (copy_tbs * 1e3), 3)
    return out


def kernel_stats(dirname):
    f = glob.glob(dirname + "/**/*kernel_stats.csv", recursive=True)[0]
    out = {}
    for r in csv.DictReader(open(f)):
        kname = r["Name"].split("(")[0].replace("void ", "")
        if "iso_" not in kname and "kuhn_" not in kname and "chunk_scan_kernel" not in kname:     # the scan of the chunk sums is shared (csrc/scan.h)
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
    ap.add_argument("--trace", help="a rocprofv3 --kernel-trace directory of the same command: adds the classify sweep's rates")
    ap.add_argument("--merge", action="store_true", help="with --trace: add the rates to the existing iso_bench.json, run nothing")
    ap.add_argument("--stats", nargs=2, metavar=("DIR", "NAME"), help="write NAME_kernel_trace.json from a --kernel-trace --stats directory")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/isosurface)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    cases = a.cases.split(",")
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "iso_bench.json")
    if a.stats:
        d, name = a.stats
        N, n, band = CASES[name]
        json.dump({"cmd": f"rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/iso_bench.py --cases {name} --reps {a.reps} --no-write; "
                          f"python tools/iso_bench.py --stats <dir> {name}",
                   "case": f"{name}: {a.reps + 1} calls of lsm_iso_create (one warm-up)", "nnode": n ** N, "kernels": kernel_stats(d)},
                  open(os.path.join(a.out, f"{name}_kernel_trace.json"), "w"), indent=1)
        return
    if a.merge:
        doc = json.load(open(path))
        rates = classify_rates(a.trace, [c["case"] for c in doc["cases"]], doc["cases"][0]["reps"], doc.get("copy_tbs_8B_per_lane"))
        for c in doc["cases"]:
            c.update(rates[c["case"]])
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    res = [run(lsm, name, a.reps) for name in cases]
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    doc = {"cmd": "python tools/iso_bench.py --reps %d" % a.reps, "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "cases": res}
    if a.trace:
        rates = classify_rates(a.trace, cases, a.reps, copy_tbs)
        for c in res:
            c.update(rates[c["case"]])
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
