#!/usr/bin/env python
"""homogenize_conductivity on the device: writes profiles/hcond/hcond_bench.json (and prints one JSON line per case).

The workload, fp64: a unit cell with a centred soft disc (radius 0.3) or ball (radius² 0.1) at contrast 1e-3, rtol 1e-8, all N
correctors from zero; at 256², 1024², 64³ and 128³ cells.
  ms_per_call       median, min, max of --reps solves of one ConductivityHomogenization after a warm-up (all N correctors, the status reads)
  ms_per_iteration  ms_per_call / Σ_k iterations_k, next to elliptic_solve's (mg) from profiles/elliptic/elliptic_bench.json at the
                    same node count where that file has one (64³ = 512², 128³) and at the nearest one otherwise, both also per
                    million nodes (the parent's measurement; another grid and another problem: an order of magnitude to hold
                    against, not a bar)
  tensor            ms of lsm_hcond_tensor (the kernel, the copy of 6 sums and the host's mirror); model bytes per cell 8·(N + 1) (the
                    cell coefficient and the N correctors, each read once from HBM), its GB/s and the fraction of the copy yardstick
  sensitivity       ms of sensitivity(W) (the cell pass and the node gather); model bytes per cell 8·(N + 1) + 24 (the cell value
                    written and read, the node value written)
  copy yardstick    --copy-tbs, or measured here: a device-to-device copy of 2^27 doubles, 8 bytes read and 8 written per element
  demo              a square cell with a round inclusion at 64² cells: the tensor, its harmonic/arithmetic bounds, the range of the
                    sensitivity of tr K^H, and three steps of an ascent on it
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

OUT = os.path.join(ROOT, "profiles", "hcond")
SIZES = {"256x256": (257, 257), "1024x1024": (1025, 1025), "64c": (65, 65, 65), "128c": (129, 129, 129)}
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


def copy_yardstick(b):
    """TB/s (read + write) of a device-to-device copy of 2^27 doubles"""
    t = b.torch
    src = t.zeros(1 << 27, dtype=t.float64, device=b.device)
    dst = t.empty_like(src)
    dst.copy_(src)
    s = timed(b, lambda: dst.copy_(src), 7)
    return round(16 * (1 << 27) / (s["ms_min"] * 1e-3) / 1e12, 2)


def against_copy(tt, cells, bytes_per_cell, copy_tbs):
    gbs = cells * bytes_per_cell / (tt["ms_min"] * 1e-3) / 1e9
    out = {**tt, "model_bytes_per_cell": bytes_per_cell, "model_gbs": round(gbs, 1)}
    if copy_tbs:
        out["frac_of_copy"] = round(gbs / (copy_tbs * 1e3), 3)
    return out


def run(lsm, name, reps, elliptic, copy_tbs):
    n = SIZES[name]
    N = len(n)
    eq, phi = field(lsm, n, inclusion(n, 0.09 if N == 2 else 0.1))
    b = phi.backend
    cells = int(np.prod([m - 1 for m in n]))
    res = {"case": name, "cells": [m - 1 for m in n], "nodes": cells, "correctors": N, "reps": reps}
    b.sync()
    t = time.perf_counter()
    hom = lsm.ConductivityHomogenization(phi)
    b.sync()
    res["create_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    hom.solve(rtol=RTOL, max_iters=5000)      # warm-up, and the first chunk's length
    s = timed(b, lambda: hom.solve(rtol=RTOL, max_iters=5000), reps)
    its = sum(hom.iterations)
    res.update({"ms_per_call": s["ms"], "ms_min": s["ms_min"], "ms_max": s["ms_max"], "iterations": hom.iterations, "relres": hom.relres, "levels": hom.levels,
                "ms_per_iteration": round(s["ms"] / its, 4), "ms_per_iteration_per_million_nodes": round(s["ms"] / its / cells * 1e6, 4)})
    if elliptic:
        e = min(elliptic.values(), key=lambda c: (abs(np.log(c["nodes"] / cells)), len(c["n"]) != N))
        res["elliptic_solve"] = {"case": e["case"], "nodes": e["nodes"], "equal_nodes": e["nodes"] == cells, "ms_per_iteration": e["mg"]["ms_per_iteration"],
                                 "ms_per_iteration_per_million_nodes": round(e["mg"]["ms_per_iteration"] / e["nodes"] * 1e6, 4)}
    h = hom._handle()
    res["tensor"] = against_copy(timed(b, lambda: b.hcond_tensor(h), max(reps, 5)), cells, 8 * (N + 1), copy_tbs)
    W = np.ones((N, N))
    res["sensitivity"] = against_copy(timed(b, lambda: hom.sensitivity(W), max(reps, 5)), cells, 8 * (N + 1) + 24, copy_tbs)
    res["K"] = hom.tensor.tolist()
    print(json.dumps(res), flush=True)
    hom.close()
    eq.backend.close()
    return res


def demo(lsm):
    """a square cell with a round inclusion: tensor, bounds, sensitivity, and three fixed-length ascent steps on tr K^H"""
    n = (65, 65)
    W = np.eye(2)
    grid = lsm.CartesianGrid((0.0, 0.0), (1.0, 1.0), n)
    state = {}

    def update(coeff, phi, t):
        hom = lsm.homogenize_conductivity(phi, rtol=RTOL, chi0=state.get("chi"))
        g = hom.sensitivity(W)
        coeff.set_values(g)
        state["chi"] = hom.correctors()
        state.setdefault("log", []).append({"t": t, "WK": float(np.sum(W * hom.tensor)), "iterations": hom.iterations})
        if "first" not in state:
            a = hom.cells()
            state["first"] = {"K": hom.tensor.tolist(), "mean_a": float(a.mean()), "harmonic_a": float(1.0 / np.mean(1.0 / a)),
                              "sensitivity_min": float(g.values().min()), "sensitivity_max": float(g.values().max())}
        hom.close()

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(inclusion(n, 0.09), grid),
                              bc=lsm.NeumannBC(), integrator=lsm.ForwardEuler())
    v0 = lsm.volume(eq)
    for _ in range(3):
        lsm.integrate_(eq, eq.current_time() + 2e-3)
    out = {"cells": [64, 64], "W": W.tolist(), **state["first"], "volume_before": float(v0), "volume_after": float(lsm.volume(eq)),
           "steps": state["log"], "note": "the speed is +sensitivity, so {phi < 0} grows fastest where W:K^H gains most: an ascent on tr K^H without a volume term; "
                   "three Forward Euler intervals of 2e-3 (update_func runs for the CFL bound and for the step: two entries per step)"}
    eq.backend.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(SIZES))
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: measured here)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/hcond)")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--refactor", metavar="PARENT_LIB", help="compare bits and speed between the parent commit's library and this one; run nothing else")
    ap.add_argument("--refactor-out", help="with --refactor: the output directory (default: profiles/cell_problem)")
    ap.add_argument("--refactor-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-demo", action="store_true")
    a = ap.parse_args()
    if a.refactor or a.refactor_child:
        import cell_problem_ab as ab
        if a.refactor:
            return ab.refactor(__file__, "hcond", a.refactor, a.reps, a.refactor_out)
        return ab.child(sys.modules[__name__], lambda lsm, phi, pc: lsm.ConductivityHomogenization(phi, precond=pc), lambda hom: hom.backend.hcond_tensor(hom._handle()), a.reps)
    import lsm_amd as lsm
    elliptic = None
    ep = os.path.join(ROOT, "profiles", "elliptic", "elliptic_bench.json")
    if os.path.exists(ep):
        elliptic = {c["case"]: c for c in json.load(open(ep))["cases"]}
    copy_tbs = a.copy_tbs
    if not copy_tbs:
        eq, phi = field(lsm, (9, 9), np.zeros((9, 9)))
        copy_tbs = copy_yardstick(phi.backend)
        eq.backend.close()
    out = {"cmd": "python tools/hcond_bench.py " + " ".join(sys.argv[1:]), "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL, "contrast": 1e-3,
           "copy_tbs": copy_tbs, "note": "first measurements; no test asserts them", "cases": [run(lsm, c, a.reps, elliptic, copy_tbs) for c in a.cases]}
    if not a.no_demo:
        out["demo"] = demo(lsm)
        print(json.dumps(out["demo"]), flush=True)
    if not a.no_write:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hcond_bench.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
