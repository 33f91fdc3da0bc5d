#!/usr/bin/env python
"""homogenize on the device: writes profiles/homogenize/homog_bench.json (and prints one JSON line per case).

The workload, fp64: a unit cell with a centred soft disc (radius 0.3) or ball (radius² 0.1) at contrast 1e-3, ν = 0.3 (plane stress
in 2-D), rtol 1e-8, all M correctors from zero; at 256², 1024², 64³ and 128³ cells.
  ms_per_call       median, min, max of --reps solves of one Homogenization after a warm-up (all M correctors, the status reads)
  ms_per_iteration  ms_per_call / Σ_k iterations_k, next to elasticity_solve's at the nearest node count from
                    profiles/elastic/elastic_bench.json (the parent's measurement; another grid and another problem: an order of
                    magnitude to hold against, not a comparison of kernels)
  tensor            ms of lsm_homog_tensor (the kernel, the copy of 21 sums and the host's mirror) and its flop model: per cell M
                    products K0·w (2·R² flops each, R = 2^N·N) and M(M+1)/2 dots (2·R + 1); multiply and add counted apart
  sensitivity       ms of sensitivity(W) (the cell pass and the node gather)
  demo              a square cell with a round hole at 64² cells: the tensor, its Reuss/Voigt bounds, the range of the
                    sensitivity of the bulk-like sum C00 + C11 + 2·C01, and three steps of an ascent on it
These are first measurements: no test asserts them.

--refactor PARENT_LIB: the parent commit's library against this one, bits and speed (tools/cell_problem_ab.py); runs nothing else."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

OUT = os.path.join(ROOT, "profiles", "homogenize")
SIZES = {"256x256": (257, 257), "1024x1024": (1025, 1025), "64c": (65, 65, 65), "128c": (129, 129, 129)}
ELASTIC = {"256x256": "512x512", "1024x1024": "2048x2048", "64c": "128c", "128c": "128c"}
RTOL = 1e-8


def inclusion(n, radius2):
    ax = [np.linspace(0.0, 1.0, m) for m in n]
    x = np.meshgrid(*ax, indexing="ij", sparse=True)
    return np.asfortranarray(radius2 - sum((xi - 0.5) ** 2 for xi in x) + np.zeros(n))


def field(lsm, n, vals):
    grid = lsm.CartesianGrid((0.0,) * len(n), (1.0,) * len(n), n)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(vals, grid), bc=lsm.NeumannBC())
    return eq, eq.current_state()


def timed(b, fn, reps):
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        fn()
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def run(lsm, name, reps, elastic):
    n = SIZES[name]
    N = len(n)
    M, R = N * (N + 1) // 2, (1 << N) * N
    eq, phi = field(lsm, n, inclusion(n, 0.09 if N == 2 else 0.1))
    b = phi.backend
    cells = int(np.prod([m - 1 for m in n]))
    res = {"case": name, "cells": [m - 1 for m in n], "nodes": cells, "unknowns": N * cells, "correctors": M, "reps": reps}
    b.sync()
    t = time.perf_counter()
    hom = lsm.Homogenization(phi)
    b.sync()
    res["create_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    hom.solve(rtol=RTOL, max_iters=5000)      # warm-up, and the first chunk's length
    s = timed(b, lambda: hom.solve(rtol=RTOL, max_iters=5000), reps)
    its = sum(hom.iterations)
    res.update({"ms_per_call": s["ms"], "ms_min": s["ms_min"], "ms_max": s["ms_max"], "iterations": hom.iterations, "relres": hom.relres, "levels": hom.levels,
                "ms_per_iteration": round(s["ms"] / its, 4)})
    if elastic and ELASTIC[name] in elastic:
        e = elastic[ELASTIC[name]]
        res["elasticity_solve"] = {"case": ELASTIC[name], "nodes": e["nodes"], "ms_per_iteration": e["mg"]["ms_per_iteration"],
                                   "ms_per_iteration_per_million_nodes": round(e["mg"]["ms_per_iteration"] / e["nodes"] * 1e6, 4)}
        res["ms_per_iteration_per_million_nodes"] = round(res["ms_per_iteration"] / cells * 1e6, 4)
    h = hom._handle()
    flops = cells * (M * 2 * R * R + M * (M + 1) // 2 * (2 * R + 1))
    tt = timed(b, lambda: b.homog_tensor(h), max(reps, 5))
    res["tensor"] = {**tt, "model_flops": flops, "model_gflops": round(flops / (tt["ms_min"] * 1e-3) / 1e9, 1)}
    W = np.ones((M, M))
    res["sensitivity"] = timed(b, lambda: hom.sensitivity(W), max(reps, 5))
    res["C"] = hom.tensor.tolist()
    print(json.dumps(res), flush=True)
    hom.close()
    eq.backend.close()
    return res


def demo(lsm):
    """a square cell with a round hole: tensor, bounds, sensitivity, and three fixed-length descent steps on W:C^H"""
    n = (65, 65)
    W = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    grid = lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), n)
    state = {}

    def update(coeff, phi, t):
        hom = lsm.homogenize(phi, rtol=RTOL, chi0=state.get("chi"))
        g = hom.sensitivity(W)
        coeff.set_values(g)
        state["chi"] = hom.correctors()
        state.setdefault("log", []).append({"t": t, "WC": float(np.sum(W * hom.tensor)), "iterations": hom.iterations})
        if "first" not in state:
            E = hom.cells()
            state["first"] = {"C": hom.tensor.tolist(), "mean_E": float(E.mean()), "harmonic_E": float(1.0 / np.mean(1.0 / E)),
                              "sensitivity_min": float(g.values().min()), "sensitivity_max": float(g.values().max())}
        hom.close()

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(inclusion(n, 0.09), grid),
                              bc=lsm.NeumannBC(), integrator=lsm.ForwardEuler())
    v0 = lsm.volume(eq)
    for _ in range(3):
        lsm.integrate_(eq, eq.current_time() + 2e-3)
    out = {"cells": [64, 64], "W": W.tolist(), **state["first"], "volume_before": float(v0), "volume_after": float(lsm.volume(eq)),
           "steps": state["log"], "note": "the speed is +sensitivity, so {phi < 0} grows fastest where W:C^H gains most: an ascent on W:C^H without a volume term; "
                   "three Forward Euler intervals of 2e-3 (update_func runs for the CFL bound and for the step: two entries per step)"}
    eq.backend.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(SIZES))
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--refactor", metavar="PARENT_LIB", help="compare bits and speed between the parent commit's library and this one; run nothing else")
    ap.add_argument("--refactor-out", help="with --refactor: the output directory (default: profiles/cell_problem)")
    ap.add_argument("--refactor-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-demo", action="store_true")
    a = ap.parse_args()
    if a.refactor or a.refactor_child:
        import cell_problem_ab as ab
        if a.refactor:
            return ab.refactor(__file__, "homog", a.refactor, a.reps, a.refactor_out)
        return ab.child(sys.modules[__name__], lambda lsm, phi, pc: lsm.Homogenization(phi, precond=pc), lambda hom: hom.backend.homog_tensor(hom._handle()), a.reps)
    import lsm_amd as lsm
    elastic = None
    ep = os.path.join(ROOT, "profiles", "elastic", "elastic_bench.json")
    if os.path.exists(ep):
        elastic = {c["case"]: c for c in json.load(open(ep))["cases"]}
    out = {"cmd": "python tools/homog_bench.py " + " ".join(sys.argv[1:]), "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL, "contrast": 1e-3, "nu": 0.3,
           "note": "first measurements; no test asserts them", "cases": [run(lsm, c, a.reps, elastic) for c in a.cases]}
    if not a.no_demo:
        out["demo"] = demo(lsm)
        print(json.dumps(out["demo"]), flush=True)
    if not a.no_write:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "homog_bench.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
