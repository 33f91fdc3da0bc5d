#!/usr/bin/env python
"""elasticity_solve on the device: writes profiles/elastic/elastic_bench.json (and prints one JSON line per case).

The workload, fp64: a plate (block) with two circular (spherical) holes as a signed distance, ersatz contrast 1e-3, ν = 0.3 (plane
stress in 2-D), clamped on the face x = 0, a uniform transverse traction on the face x = 1 (f = 2t/h_x on its nodes), rtol 1e-8, from
a zero guess; at 512² and 2048², 128³ and 256³.
  mg / jacobi     ms_per_solve (median, min, max of --reps solves of one ElasticityOperator after a warm-up solve: the fields for u,
                  the kernels, the status reads and the store), iterations, relres, ms_per_iteration; create_ms: the hierarchy
  ms_per_vcycle   mg's ms_per_iteration minus jacobi's (an estimate: jacobi's K2 also writes z); the traced run has the kernels
  model           DESIGN.md §7.18's count per node and apply: flops (2·(2^N·N)²·... multiply and add, not contracted) and bytes; the
                  apply's gflops = model flops · nodes · applies per iteration / ms_per_iteration, an upper bound on what the
                  applies reach since the other kernels take time too
  copy_tbs        tools/copy_bw's 8-bytes-per-lane copy of the same run (`--copy-tbs` to give it instead)
Kernel shares: run `--no-write --only NAME --precond mg` under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, a run
of its own, then `--stats DIR --only NAME` adds every es_* and mg_* kernel's dispatches, total time and share to the file.
Comparing two builds: a library built elsewhere (make OBJDIR=… OUT=…) is loaded with LSM_AMD_LIB; `--no-write --only NAME --precond mg`
with each library in turn is how DESIGN.md §7.18 compared loading each neighbour value where a cell uses it (removed since).  `--table` prints the restatement's iteration table (tests/_elastic_ref.py), no device needed."""
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

OUT = os.path.join(ROOT, "profiles", "elastic")
SIZES = {"512x512": (512, 512), "2048x2048": (2048, 2048), "128c": (128, 128, 128), "256c": (256, 256, 256)}
RTOL = 1e-8


def model(N, precond):
    """per node: the flops of one apply (multiply and add counted apart: no contraction) and the applies per iteration on level 0"""
    R = (1 << N) * N
    flops = (1 << N) * (2 * N * R + 2 * N)                      # per cell: N rows of R multiply-adds, then ·E and the sum
    applies = 1 + (4 / (1 - 2.0 ** -N) if precond == "mg" else 0)      # K1; the V-cycle: 3 sweeps with an apply and the residual, per level
    return flops, applies


def two_holes(n):
    ax = [np.linspace(0.0, 1.0, m) for m in n]
    x = np.meshgrid(*ax, indexing="ij", sparse=True)
    c1 = (0.3, 0.35, 0.5)[:len(n)]
    c2 = (0.7, 0.65, 0.4)[:len(n)]
    d1 = np.sqrt(sum((xi - c) ** 2 for xi, c in zip(x, c1))) - 0.17
    d2 = np.sqrt(sum((xi - c) ** 2 for xi, c in zip(x, c2))) - 0.17
    return np.asfortranarray(-np.minimum(d1, d2) + np.zeros(n))


def summary(ts, key="ms_per_solve"):
    return {key: round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def field(lsm, n, vals):
    grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid), bc=lsm.NeumannBC())
    return eq, eq.current_state()


def load(b, n):
    """the traction (0, −1, 0…) on the face x = 1 as one flat device array, component-major"""
    t = b.torch
    N = len(n)
    nn = int(np.prod(n))
    f = t.zeros(N * nn, dtype=t.float64, device=b.device)
    face = t.arange(n[0] - 1, nn, n[0], device=b.device)
    f[nn + face] = -2.0 * (n[0] - 1)
    return f


def run(lsm, name, reps, preconds):
    n = SIZES[name]
    N = len(n)
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    res = {"case": name, "n": list(n), "nodes": int(np.prod(n)), "unknowns": N * int(np.prod(n)), "reps": reps}
    f = load(b, n)
    for pc in preconds:
        b.sync()
        t = time.perf_counter()
        op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond=pc)
        b.sync()
        create_ms = (time.perf_counter() - t) * 1e3
        sol = op.solve(f, rtol=RTOL, max_iters=200000)       # warm-up, and the first chunk's length
        ts = []
        for _ in range(reps):
            b.sync()
            t = time.perf_counter()
            sol = op.solve(f, rtol=RTOL, max_iters=200000)
            b.sync()
            ts.append((time.perf_counter() - t) * 1e3)
        r = {**summary(ts), "iterations": sol.iterations, "relres": sol.relres, "levels": sol.levels, "create_ms": round(create_ms, 3),
             "compliance": sol.compliance()}
        r["ms_per_iteration"] = round(r["ms_per_solve"] / sol.iterations, 4)
        flops, applies = model(N, pc)
        r["model_flops_per_node_apply"], r["model_applies_per_iteration"] = flops, round(applies, 3)
        r["apply_gflops_bound"] = round(flops * applies * res["nodes"] / (r["ms_per_iteration"] * 1e-3) / 1e9, 1)
        res[pc] = r
        del sol
        op.close()
    if "mg" in res and "jacobi" in res:
        res["ms_per_vcycle"] = round(res["mg"]["ms_per_iteration"] - res["jacobi"]["ms_per_iteration"], 4)
    print(json.dumps(res), flush=True)
    eq.backend.close()
    return res


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
        m = re.search(r"\b(es|mg)_\w+_kernel(<[\w:, ]+>)?", r["Name"].split("(")[0])
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


def table():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _elastic_ref as R
    print("grid levels  V-cycle ω ≤ 0.6  ω ≤ 0.8  fixed ω = 0.6  Jacobi")
    for n, hc in R.TABLE:
        row = []
        for pc, om, fixed in (("mg", 0.6, False), ("mg", 0.8, False), ("mg", 0.6, True), ("jacobi", 0.6, False)):
            hier, f, u0 = R.prototype(n, hc, fixed_omega=fixed)
            u, it, rel, ok = R.pcg(hier, f, u0, 1e-8, 3000, pc, om)
            row.append(it if ok else "no convergence in 3000")
        print("x".join(map(str, n)), hier.levels, *row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--only", choices=list(SIZES), help="one case (the run under the profiler, or with --stats the case the trace is of)")
    ap.add_argument("--precond", choices=("mg", "jacobi"), help="with --only: one preconditioner")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the es_* kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--table", action="store_true", help="print the restatement's iteration table and exit")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/elastic)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    if a.table:
        table()
        return
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "elastic_bench.json")
    if a.stats:
        doc = json.load(open(path))
        tr = doc.setdefault("kernel_trace", {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/elastic_bench.py --no-write "
                                                    "--only NAME --precond mg; python tools/elastic_bench.py --stats <dir> --only NAME",
                                             "note": "one traced run, the hierarchy's setup and the warm-up solve included (traced, so slower than the plain run)",
                                             "cases": {}})
        tr["cases"][a.only] = kernel_stats(a.stats)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, a.reps, (a.precond,) if a.precond else ("mg", "jacobi"))
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    doc = {"cmd": "python tools/elastic_bench.py --reps %d --cases %s" % (a.reps, " ".join(a.cases)), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "rtol": RTOL, "contrast": 1e-3, "nu": 0.3, "cases": []}
    for name in a.cases:        # the file is rewritten after every case: the largest one may be cut short
        doc["cases"].append(run(lsm, name, a.reps, ("mg", "jacobi")))
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)

if __name__ == "__main__":
    main()
