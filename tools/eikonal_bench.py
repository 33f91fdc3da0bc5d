#!/usr/bin/env python
"""eikonal_ on the device: writes profiles/eikonal/eikonal_bench.json (and prints one JSON line per case).

The workload: the sphere of radius 0.5 in [−1, 1]³ at 96³, 256³ and 512³, redistanced over the whole grid, with both seedings:
  crossing   ϕ = |x|² − 0.25 (not a distance: reinit_bench.py's input), seeded from the crossings along the grid lines
  width      ϕ = |x| − 0.5, the nodes with |ϕ| <= 1.5h frozen at |ϕ|
  ms_per_call       wall time of one synchronous lsm_eikonal (seed kernel and its host read, the tile launches with one host read of
                    the list length each, the final pass, the host read of the statistics): median, min and max of --reps calls
                    after the warm-up calls (at least two, and at least 100 ms of them); ϕ is restored from a copy before each
                    call, outside the timed window
  iterations        outer iterations (launches of the tile kernel); visits: tiles visited over all of them
  nodes_per_s       grid nodes / ms_per_call: what a caller gets
  tile_nodes_per_s  visits × 512 nodes / ms_per_call: what the tile kernel sustains, passes and host reads included
  max_err           max |ϕ − (|x| − 0.5)| in units of h
and at 96³ the only other whole-grid route, reinitialize_ on the dense field with the same input, call by call interleaved with
the crossing-seed eikonal_.

Kernel shares: run the same command with --no-write --only N under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`,
then `--stats DIR` adds every ek_* kernel's dispatches and total time, their shares, and the final pass's rate under its traffic
model (8 bytes of T and 8 of ϕ read, 8 written per node) against `--copy-tbs`, what tools/copy_bw reaches with 8 bytes per lane
(read + write; the tool is run when the option is absent and the program is built).

What was tried: `--variants LABEL=LIB …` measures one grid with libraries built with other constants (csrc/lsm_eikonal.hip:
-DLSM_EK_PASSES, -DLSM_EK_TX/TY/TZ), one process per library, the libraries taken in turn."""
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
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

OUT = os.path.join(ROOT, "profiles", "eikonal")
FINAL_BYTES_PER_NODE = 24
TILE_NODES = 512


def fields(lsm, n):
    """(the state holding |x|² − 0.25, a device copy of it, a device copy of |x| − 0.5, |x| − 0.5 on the host)"""
    grid = lsm.CartesianGrid((-1.0,) * 3, (1.0,) * 3, (n,) * 3)
    ax = np.linspace(-1.0, 1.0, n)
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    exact = np.asfortranarray(np.sqrt(r2) - 0.5)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.asfortranarray(r2 - 0.25), grid), bc=lsm.ExtrapolationBC(2))
    st = eq.current_state()
    quad = st.buf.clone()
    dist = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(exact, grid), bc=lsm.ExtrapolationBC(2)).current_state().buf.clone()
    return eq, st, quad, dist, exact


def interleaved(b, st, reps, calls):
    """calls: name → (the buffer ϕ is restored from, the call); every round runs each once, in turn.  Returns name → [ms]"""
    ts = {k: [] for k in calls}
    warm, t_warm = 0, time.perf_counter()
    while warm < 2 or time.perf_counter() - t_warm < 0.1:
        for src, call in calls.values():
            st.buf.copy_(src)
            call()
        b.sync()
        warm += 1
    for _ in range(reps):
        for k, (src, call) in calls.items():
            st.buf.copy_(src)
            b.sync()
            t = time.perf_counter()
            call()
            b.sync()
            ts[k].append((time.perf_counter() - t) * 1e3)
    return ts


def summary(ts):
    return {"ms_per_call": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def run(lsm, n, reps, with_reinit):
    eq, st, quad, dist, exact = fields(lsm, n)
    b = st.backend
    h = 2.0 / (n - 1)
    stats = {}
    calls = {"crossing": (quad, lambda: stats.__setitem__("crossing", b.eikonal(st.buf, None, 0.0, float("inf"), 0))),
             "width": (dist, lambda: stats.__setitem__("width", b.eikonal(st.buf, None, 1.5 * h, float("inf"), 0)))}
    if with_reinit:
        calls["reinitialize_dense"] = (quad, lambda: lsm.reinitialize_(st))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts = interleaved(b, st, reps, calls)
        out = []
        for k, (src, call) in calls.items():
            st.buf.copy_(src)
            call()
            err = float(np.abs(st.values() - exact).max()) / h
            res = {"case": f"sphere{n}", "n": n, "what": k, "reps": reps, **summary(ts[k]), "max_err_h": round(err, 6)}
            if k in stats:
                frozen, iters, visits, _ = stats[k]
                ms = res["ms_per_call"]
                res.update({"frozen_nodes": frozen, "iterations": iters, "visits": visits, "tiles": ((n + 7) // 8) ** 3,
                            "nodes_per_s": round(n ** 3 / (ms * 1e-3)), "tile_nodes_per_s": round(visits * TILE_NODES / (ms * 1e-3))})
            print(json.dumps(res), flush=True)
            out.append(res)
    eq.backend.close()
    return out


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
        m = re.search(r"\bek_\w+_kernel", r["Name"].split("(")[0])
        if not m:
            continue
        kname = m.group(0)
        e = out.setdefault(kname, {"dispatches": 0, "total_ms": 0.0})
        e["dispatches"] += int(r["Calls"])
        e["total_ms"] += int(r["TotalDurationNs"]) / 1e6
    total = sum(e["total_ms"] for e in out.values())
    for e in out.values():
        e["share"] = round(e["total_ms"] / total, 4)
        e["total_ms"] = round(e["total_ms"], 3)
        e["us_per_dispatch"] = round(1e3 * e["total_ms"] / e["dispatches"], 2)
    return out


def run_variants(specs, n, reps, rounds):
    """label=path …: the same --only run in a process of its own per library (LSM_AMD_LIB), the libraries taken in turn `rounds`
    times; returns label → {seeding → {ms: [one median per round], iterations, visits}}"""
    out = {}
    for _ in range(rounds):
        for spec in specs:
            label, path = spec.split("=", 1)
            env = dict(os.environ, LSM_AMD_LIB=os.path.abspath(path))
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", str(n), "--no-write", "--reps", str(reps)], env=env,
                                 capture_output=True, text=True, timeout=600, check=True).stdout
            for line in txt.splitlines():
                if not line.startswith("{"):
                    continue
                r = json.loads(line)
                e = out.setdefault(label, {"lib": path}).setdefault(r["what"], {"ms": [], "iterations": r["iterations"], "visits": r["visits"],
                                                                               "max_err_h": r["max_err_h"]})
                e["ms"].append(r["ms_per_call"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", metavar="LABEL=LIB", help="add the --variants-n case measured with each of these libraries to the existing file")
    ap.add_argument("--variants-n", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2, help="--variants: times each library is taken, in turn")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 256, 512])
    ap.add_argument("--only", type=int, help="one size, no reinitialize_ (the run under the profiler: every dispatch is that grid's)")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the ek_* kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--stats-n", type=int, default=256, help="the grid the traced run used (--only)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/eikonal)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "eikonal_bench.json")
    if a.variants:
        doc = json.load(open(path))
        doc["variants"] = {"n": a.variants_n, "reps": a.reps, "rounds": a.rounds,
                           "note": "one process per library and round (LSM_AMD_LIB), libraries taken in turn; ms: the median of each round",
                           "libraries": run_variants(a.variants, a.variants_n, a.reps, a.rounds)}
        json.dump(doc, open(path, "w"), indent=1)
        print(json.dumps(doc["variants"]["libraries"]))
        return
    if a.stats:
        doc = json.load(open(path))
        ks = kernel_stats(a.stats)
        doc["kernel_trace"] = {"cmd": f"rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/eikonal_bench.py --no-write --only {a.stats_n}; "
                                      f"python tools/eikonal_bench.py --stats <dir> --stats-n {a.stats_n}",
                               "n": a.stats_n, "note": "both seedings, warm-up calls included (traced, so slower than the plain run)", "kernels": ks}
        fin = ks.get("ek_final_kernel")
        if fin:
            gbs = FINAL_BYTES_PER_NODE * a.stats_n ** 3 / (fin["us_per_dispatch"] * 1e-6) / 1e9
            doc["kernel_trace"]["final_model_gbs"] = round(gbs, 1)
            if doc.get("copy_tbs_8B_per_lane"):
                doc["kernel_trace"]["final_frac_of_copy"] = round(gbs / (doc["copy_tbs_8B_per_lane"] * 1e3), 3)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, a.reps, False)
        return
    cases = []
    for n in a.sizes:
        cases += run(lsm, n, a.reps, n == 96)
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    doc = {"cmd": "python tools/eikonal_bench.py --reps %d" % a.reps, "device": "MI355X (gfx950), 1 GPU", "copy_tbs_8B_per_lane": copy_tbs,
           "final_model_bytes_per_node": FINAL_BYTES_PER_NODE, "tile": [8, 8, 8], "passes_per_visit": 8, "cases": cases}
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
