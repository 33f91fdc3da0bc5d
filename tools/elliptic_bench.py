#!/usr/bin/env python
"""elliptic_solve on the device: writes profiles/elliptic/elliptic_bench.json (and prints one JSON line per case).

The workload, fp64: a plate (block) with two circular (spherical) holes as a signed distance, ersatz contrast 1e-3, f = 1, u = 0 on
the face x = 0, rtol 1e-8, from a zero guess; at 512² and 2048², 128³ and 256³.
  mg / jacobi     ms_per_solve (median, min, max of --reps solves of one EllipticOperator after a warm-up solve: the field for u,
                  the kernels, the status reads and the store), iterations, relres, ms_per_iteration; create_ms: the hierarchy
  ms_per_vcycle   mg's ms_per_iteration minus jacobi's: an estimate (jacobi's K2 also writes z); the traced run has the kernels
  model_gbs       MODEL bytes per node and iteration · nodes / ms_per_iteration, against `--copy-tbs` (tools/copy_bw, 8 bytes per
                  lane, read + write; run when the option is absent and the program is built).  The model, level 0,
                  fixed mask of 1 byte included: K1 41 (z, p, cells, mask read; p', q written), K2 48 (x, r, p', q read; x, r
                  written), jacobi's K2 64 (D read, z written as well); the V-cycle on level 0: first sweep 25, three sweeps of 41,
                  residual 33 and its restriction 8 + 8/2^N, prolong-and-correct 17 + 8/2^N; the coarser levels add the factor 1/(1 − 2^−N)
  regularize      regularize_ of a random field at α = 4h: ms_per_call, iterations
Kernel shares: run `--no-write --only NAME --precond mg` under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, a run
of its own, then `--stats DIR --only NAME` adds every el_* and mg_* kernel's dispatches, total time and share to the file.
Comparing two builds: a library built elsewhere (make OBJDIR=… OUT=…) is loaded with LSM_AMD_LIB; `--no-write --only NAME --precond mg`
with each library in turn is how DESIGN.md §7.17 compared the one-kernel residual-and-restrict (removed since) with the two-pass form.
--demo: a small 2-D thermal-compliance descent (NormalMotionTerm whose update_func solves the state equation and sets the normal
speed to e − ℓ, the descent direction of compliance + ℓ·volume for ϕ_t + v|∇ϕ| = 0; reinitialize_ every few steps); records the
objective per outer step into the same file."""
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

OUT = os.path.join(ROOT, "profiles", "elliptic")
SIZES = {"512x512": (512, 512), "2048x2048": (2048, 2048), "128c": (128, 128, 128), "256c": (256, 256, 256)}
RTOL = 1e-8


def model_bytes(N, precond):
    k1, k2 = 41.0, 48.0 if precond == "mg" else 64.0
    if precond != "mg":
        return k1 + k2
    level0 = 25 + 3 * 41 + (33 + 8 + 8 / 2 ** N) + (17 + 8 / 2 ** N)
    return k1 + k2 + level0 / (1 - 2.0 ** -N)


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


def run(lsm, name, reps, preconds):
    n = SIZES[name]
    N = len(n)
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    res = {"case": name, "n": list(n), "nodes": int(np.prod(n)), "reps": reps}
    for pc in preconds:
        b.sync()
        t = time.perf_counter()
        op = lsm.EllipticOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond=pc)
        b.sync()
        create_ms = (time.perf_counter() - t) * 1e3
        f = b.node_array(1.0, "f")
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
        r["model_bytes_per_node"] = round(model_bytes(N, pc), 1)
        r["model_gbs"] = round(r["model_bytes_per_node"] * res["nodes"] / (r["ms_per_iteration"] * 1e-3) / 1e9, 1)
        res[pc] = r
        op.close()
    if "mg" in res and "jacobi" in res:
        res["ms_per_vcycle"] = round(res["mg"]["ms_per_iteration"] - res["jacobi"]["ms_per_iteration"], 4)
    if "mg" in preconds:
        g0 = np.asfortranarray(np.random.default_rng(1).standard_normal(n))
        g = lsm.ROCMeshField(b, phi.mesh, phi.bcs, b.clone(phi.buf))
        ts = []
        for _ in range(max(2, reps // 2) + 1):
            b.upload(g.buf, g0)
            b.sync()
            t = time.perf_counter()
            sol = lsm.regularize_(g, 4.0 / (n[0] - 1), rtol=RTOL)
            b.sync()
            ts.append((time.perf_counter() - t) * 1e3)
        res["regularize"] = {**summary(ts[1:], "ms_per_call"), "alpha_over_h": 4, "iterations": sol.iterations, "relres": sol.relres}
    print(json.dumps(res), flush=True)
    eq.backend.close()
    return res


def demo(lsm, m=129, steps=12, reinit_every=4):
    n = (m, m)
    eq0, phi0 = field(lsm, n, two_holes(n))
    grid = phi0.mesh
    h = min(grid.meshsize())
    patch = lsm.face_mask(grid, 0, 0)
    patch[:, : m // 3] = False
    patch[:, 2 * m // 3:] = False
    state = {}

    def solve(phi):
        sol = lsm.elliptic_solve(phi, 1.0, dirichlet=(patch, 0.0), rtol=RTOL)
        e = sol.energy_density()
        state["compliance"], state["iterations"] = sol.compliance(), sol.iterations
        sol.operator.close()
        return e

    e = solve(phi0)
    inside = phi0.values() < 0
    ell = float(e.values()[inside].mean())
    vmax = float(np.abs(e.values() - ell).max())
    eq0.backend.close()

    def update(coeff, phi, t):
        e = solve(phi)
        e.buf.sub_(ell)                   # the speed e − ℓ, on the device
        coeff.set_values(e)

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(two_holes(n), grid),
                              bc=lsm.NeumannBC(), integrator=lsm.RK3())
    hist = []
    tau = h / vmax
    for k in range(steps):
        solve(eq.current_state())
        hist.append({"step": k, "compliance": state["compliance"], "volume": lsm.volume(eq), "pcg_iterations": state["iterations"]})
        hist[-1]["objective"] = hist[-1]["compliance"] + ell * hist[-1]["volume"]
        print(json.dumps(hist[-1]), flush=True)
        lsm.integrate_(eq, eq.current_time() + tau)
        if (k + 1) % reinit_every == 0:
            lsm.reinitialize_(eq.current_state())
    eq.backend.close()
    return {"grid": list(n), "ell": ell, "outer_step": "one cell at the first step's largest speed", "reinitialize_every": reinit_every, "history": hist}


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
        m = re.search(r"\b(el_\w+_kernel|mg_\w+_kernel(<[\w:, ]+>)?)", r["Name"].split("(")[0])
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--only", choices=list(SIZES), help="one case (the run under the profiler, or with --stats the case the trace is of)")
    ap.add_argument("--precond", choices=("mg", "jacobi"), help="with --only: one preconditioner")
    ap.add_argument("--demo", action="store_true", help="run the thermal-compliance descent and add its history to the file")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the el_* kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/elliptic)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "elliptic_bench.json")
    if a.stats:
        doc = json.load(open(path))
        tr = doc.setdefault("kernel_trace", {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/elliptic_bench.py --no-write "
                                                    "--only NAME --precond mg; python tools/elliptic_bench.py --stats <dir> --only NAME",
                                             "note": "one traced run, the hierarchy's setup and the warm-up solve included (traced, so slower than the plain run)",
                                             "cases": {}})
        tr["cases"][a.only] = kernel_stats(a.stats)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, a.reps, (a.precond,) if a.precond else ("mg", "jacobi"))
        return
    doc = {}
    cases = [run(lsm, name, a.reps, ("mg", "jacobi")) for name in a.cases]
    dm = demo(lsm) if a.demo else None
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        for r in cases:
            for pc in ("mg", "jacobi"):
                r[pc]["frac_of_copy"] = round(r[pc]["model_gbs"] / (copy_tbs * 1e3), 3)
    doc.update({"cmd": "python tools/elliptic_bench.py --reps %d%s" % (a.reps, " --demo" if a.demo else ""), "device": "MI355X (gfx950), 1 GPU",
                "copy_tbs_8B_per_lane": copy_tbs, "rtol": RTOL, "contrast": 1e-3, "cases": cases})
    if dm:
        doc["demo"] = dm
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
