#!/usr/bin/env python
"""components on the device: writes profiles/components/cc_bench.json (and prints one JSON line per case).

The workload, fp64, on [−1, 1]³ at 96³, 256³ and 512³:
  sphere      |x| − 0.5: one large component
  spheres8    an 8 × 8 × 8 array of spheres of radius 0.08 (512 components)
  random      uniform values − 0.20, the fraction of tests/test_gpu_components.py's many_tiles: clusters of every size sprawling
              over the tiles, the merge's worst case
  all_inside  every node in one component: the statistics' worst case (every tile adds to the same ten words)
  ms_per_call     wall time of one components(ϕ) + close(): lsm_cc_create (its kernels and its one host read), lsm_cc_read (the
                  labels copied device to device, the statistics brought to the host) and lsm_cc_destroy; median, min and max of
                  --reps calls after the warm-up calls (at least two, and at least 100 ms of them), the cases taken in turn
  K, set_nodes, cross_tile_edges   lsm_cc_create's stats
  model_gbs       MODEL_BYTES_PER_NODE · nodes / ms_per_call: the bytes every node costs at least — 8 of ϕ read and 4 of parent
                  written (cc_local), 4 read and 4 written (cc_flatten), 4 read (cc_number), 4 of parent read and 4 of labels
                  written (cc_label), 4 + 4 for lsm_cc_read's copy of the labels — without the walks of cc_merge and cc_flatten
                  and cc_label's gather of the root's label; frac_of_copy: against `--copy-tbs`, what tools/copy_bw reaches in the
                  same run with 8 bytes per lane (read + write; the tool is run when the option is absent and the program is built)
and with --scipy, at 256³, the route this replaces: ϕ.values() + scipy.ndimage.label with the Kuhn structure element.

Kernel shares: run `--no-write --only N --case NAME` under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, a run of
its own, then `--stats DIR --stats-n N --case NAME` adds every cc_* kernel's dispatches, total time and share to the file."""
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

OUT = os.path.join(ROOT, "profiles", "components")
MODEL_BYTES_PER_NODE = 40
FRACTION = 0.20
CASES = ("sphere", "spheres8", "random", "all_inside")


def values(case, n):
    ax = np.linspace(-1.0, 1.0, n)
    if case == "sphere":
        return np.asfortranarray(np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5)
    if case == "spheres8":
        d = (np.abs(((ax + 1.0) % 0.25) - 0.125)) ** 2           # squared distance to the nearest centre along one axis
        return np.asfortranarray(np.sqrt(d[:, None, None] + d[None, :, None] + d[None, None, :]) - 0.08)
    if case == "random":
        return np.asfortranarray(np.random.default_rng(7).random((n, n, n)) - FRACTION)
    return np.asfortranarray(np.full((n, n, n), -1.0))


def summary(ts):
    return {"ms_per_call": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def run(lsm, n, reps, cases, scipy_too=False):
    grid = lsm.CartesianGrid((-1.0,) * 3, (1.0,) * 3, (n,) * 3)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(values(cases[0], n), grid), bc=lsm.NeumannBC())
    st = eq.current_state()
    b = st.backend
    fields = {}
    for case in cases:
        f = lsm.ROCMeshField(b, st.mesh, st.bcs, b.clone(st.buf))
        b.upload(f.buf, values(case, n))
        fields[case] = f

    def call(f):
        c = lsm.components(f)
        stats = c.stats
        c.close()
        return stats

    ts, stats = {k: [] for k in cases}, {}
    warm, t_warm = 0, time.perf_counter()
    while warm < 2 or time.perf_counter() - t_warm < 0.1:
        for f in fields.values():
            call(f)
        b.sync()
        warm += 1
    for _ in range(reps):
        for k, f in fields.items():
            b.sync()
            t = time.perf_counter()
            stats[k] = call(f)
            b.sync()
            ts[k].append((time.perf_counter() - t) * 1e3)
    out = []
    for k in cases:
        res = {"case": f"{k}{n}", "n": n, "what": k, "reps": reps, **summary(ts[k]), "K": stats[k][0], "set_nodes": stats[k][1],
               "cross_tile_edges": stats[k][2], "tiles": ((n + 7) // 8) ** 3}
        res["nodes_per_s"] = round(n ** 3 / (res["ms_per_call"] * 1e-3))
        res["model_gbs"] = round(MODEL_BYTES_PER_NODE * n ** 3 / (res["ms_per_call"] * 1e-3) / 1e9, 1)
        print(json.dumps(res), flush=True)
        out.append(res)
    host = None
    if scipy_too:
        try:
            import scipy.ndimage as ndi
        except ImportError:
            host = {"n": n, "note": "scipy is not installed on this machine: no comparison"}
        else:
            s = np.zeros((3, 3, 3), dtype=bool)
            for d in np.ndindex(2, 2, 2):
                s[tuple(1 + k for k in d)] = s[tuple(1 - k for k in d)] = True
            f, hs = fields["random" if "random" in fields else cases[0]], []
            for _ in range(3):
                t = time.perf_counter()
                _, K = ndi.label(f.values() < 0.0, structure=s)
                hs.append((time.perf_counter() - t) * 1e3)
            host = {"n": n, "what": "values() + scipy.ndimage.label(structure = Kuhn), the random case", "K": int(K), **summary(hs)}
        print(json.dumps(host), flush=True)
    eq.backend.close()
    return out, host


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
        m = re.search(r"\b(cc_\w+|chunk_scan)_kernel", r["Name"].split("(")[0])      # chunk_scan: the shared scan (csrc/scan.h)
        if not m:
            continue
        e = out.setdefault(m.group(0), {"dispatches": 0, "total_ms": 0.0})
        e["dispatches"] += int(r["Calls"])
        e["total_ms"] += int(r["TotalDurationNs"]) / 1e6
    total = sum(e["total_ms"] for e in out.values())
    for e in out.values():
        e["share"] = round(e["total_ms"] / total, 4)
        e["total_ms"] = round(e["total_ms"], 3)
        e["us_per_dispatch"] = round(1e3 * e["total_ms"] / e["dispatches"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 256, 512])
    ap.add_argument("--only", type=int, help="one size (the run under the profiler: every dispatch is that grid's)")
    ap.add_argument("--case", choices=CASES, help="with --only or --stats: one case")
    ap.add_argument("--scipy", action="store_true", help="at 256³, time values() + scipy.ndimage.label too")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the cc_* kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--stats-n", type=int, default=256, help="the grid the traced run used (--only)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/components)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "cc_bench.json")
    if a.stats:
        doc = json.load(open(path))
        tr = doc.setdefault("kernel_trace", {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cc_bench.py --no-write "
                                                    "--only N --case NAME; python tools/cc_bench.py --stats <dir> --stats-n N --case NAME",
                                             "note": "one traced run per case, warm-up calls included (traced, so slower than the plain run)", "cases": {}})
        tr["cases"][f"{a.case}{a.stats_n}"] = kernel_stats(a.stats)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, a.reps, (a.case,) if a.case else CASES)
        return
    cases, host = [], None
    for n in a.sizes:
        res, hst = run(lsm, n, a.reps, CASES, a.scipy and n == 256)
        cases += res
        host = hst or host
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        for r in cases:
            r["frac_of_copy"] = round(r["model_gbs"] / (copy_tbs * 1e3), 3)
    doc = {"cmd": "python tools/cc_bench.py --reps %d%s" % (a.reps, " --scipy" if a.scipy else ""), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "model_bytes_per_node": MODEL_BYTES_PER_NODE, "tile": [8, 8, 8], "random_fraction": FRACTION, "cases": cases}
    if host:
        doc["host_route"] = host
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
