#!/usr/bin/env python
"""Stress recovery on the device: writes profiles/stress/stress_bench.json (and prints one JSON line per case).

The workload, fp64: elastic_bench's cantilever (a block with two holes as a signed distance, contrast 1e-3, ν = 0.3, clamped on x = 0,
a transverse traction on x = 1) at 2048², 128³ and 256³, solved once at rtol 1e-8; then, per call (median, min, max of --reps after a
warm-up, the stream synchronised around each):
  fields        strain(), stress(), von_mises(): the cell pass into scratch and the node gather, new fields included
  norm          lsm_elastic_stress_norm (J′ and smax, one pass, synchronous)
  load          lsm_elastic_stress_load (the cell pass and the gather)
  sensitivity   lsm_elastic_stress_sensitivity (the cell pass with the 2^N·N-square bilinear form, and the gather)
  model_gbs     MODEL bytes / ms, against `--copy-tbs` (tools/copy_bw's 8-bytes-per-lane copy of the same run, read + write, when the
                option is absent and the program is built).  The model counts every array once, 8 bytes an entry: the N fields of u
                and the cell moduli read (the strain reads no moduli), what the cell pass leaves in scratch written and read again, the
                M (or 1, or N) results written; the sensitivity reads the N adjoint fields as well.
  adjoint       stress_sensitivity(p = 8) end to end: ms, and the adjoint solve's iterations next to the state solve's
--demo: an L-bracket built from two boxes (clamped on top, a downward traction on the end of the arm): smax, the cell where it sits (at
the re-entrant corner), the compliance and G_p for p = 4, 8, 16, into the same file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from elastic_bench import copy_yardstick, field, load, two_holes

OUT = os.path.join(ROOT, "profiles", "stress")
SIZES = {"2048x2048": (2048, 2048), "128c": (128, 128, 128), "256c": (256, 256, 256)}
RTOL, P = 1e-8, 8.0


def model_bytes(N, n):
    """bytes per call of each pass: nodes·8·(node arrays) + cells·8·(cell arrays)"""
    M = N * (N + 1) // 2
    nodes, cells = float(np.prod(n)), float(np.prod([m - 1 for m in n]))
    w = lambda na, ca: 8.0 * (na * nodes + ca * cells)
    return {"strain": w(N + M, 2 * M), "stress": w(N + M, 1 + 2 * M), "von_mises": w(N + 1, 1 + 2), "norm": w(N, 1), "load": w(2 * N, 1 + 2 * (1 + M)),
            "sensitivity": w(2 * N + 1, 1 + 2)}


def timed(b, reps, call):
    call()
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        call()
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"ms_per_call": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def run(lsm, name, reps):
    n = SIZES[name]
    N = len(n)
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    sol = op.solve(load(b, n), rtol=RTOL, max_iters=200000)
    h, ub = op._handle(), [c.buf for c in sol.u]
    smax = sol.stress_max()
    res = {"case": name, "n": list(n), "nodes": int(np.prod(n)), "reps": reps, "state_iterations": sol.iterations, "smax": smax,
           "G_p": {str(int(p)): sol.stress_norm(p) for p in (4.0, 8.0, 16.0)}}
    t = time.perf_counter()
    sens = sol.stress_sensitivity(p=P, rtol=RTOL, max_iters=200000)
    b.sync()
    res["adjoint"] = {"p": P, "ms_stress_sensitivity": round((time.perf_counter() - t) * 1e3, 3), "iterations": sens.iterations, "state_iterations": sol.iterations}
    lb, g = [c.buf for c in sens.adjoint.u], sens.field
    calls = {"strain": sol.strain, "stress": sol.stress, "von_mises": sol.von_mises, "norm": lambda: b.elastic_stress_norm(h, ub, P, smax),
             "load": lambda: b.elastic_stress_load(h, ub, P, smax), "sensitivity": lambda: b.elastic_stress_sensitivity(h, ub, lb, P, smax, 1.0, g.buf)}
    mb = model_bytes(N, n)
    for key, call in calls.items():
        r = timed(b, reps, call)
        r["model_bytes"] = mb[key]
        r["model_gbs"] = round(mb[key] / (r["ms_per_call"] * 1e-3) / 1e9, 1)
        res[key] = r
    print(json.dumps(res), flush=True)
    del sol, sens
    op.close()
    eq.backend.close()
    return res


def demo(lsm, m=129):
    """an L-bracket from two boxes: the column x ≤ 0.4 and the arm y ≤ 0.4 of the unit square; ϕ < 0 inside either"""
    n = (m, m)
    ax = np.linspace(0.0, 1.0, m)
    x, y = np.meshgrid(ax, ax, indexing="ij")
    box = lambda x0, x1, y0, y1: np.maximum(np.maximum(x0 - x, x - x1), np.maximum(y0 - y, y - y1))
    vals = np.asfortranarray(np.minimum(box(-1.0, 0.4, -1.0, 2.0), box(-1.0, 2.0, -1.0, 0.4)))
    eq, phi = field(lsm, n, vals)
    b = phi.backend
    clamp = lsm.face_mask(phi.mesh, 1, 1) & (x <= 0.4)
    f = np.zeros((2,) + n)
    f[1][(x == 1.0) & (y <= 0.4)] = -2.0 * (m - 1)
    sol = lsm.elasticity_solve(phi, f, dirichlet=(clamp, 0.0), rtol=RTOL)
    vm = sol.von_mises().values()
    cells = b.elastic_stress_cells(sol.operator._handle(), [c.buf for c in sol.u], lsm._lib.STRESS_VON_MISES).cpu().numpy().reshape((m - 1, m - 1), order="F")
    at = np.unravel_index(int(np.argmax(cells)), cells.shape)
    e = sol.energy_density().values()
    out = {"grid": list(n), "iterations": sol.iterations, "compliance": sol.compliance(), "smax": sol.stress_max(),
           "smax_cell_centre": [round((at[0] + 0.5) / (m - 1), 4), round((at[1] + 0.5) / (m - 1), 4)], "re_entrant_corner": [0.4, 0.4],
           "von_mises_node_max": float(vm.max()), "energy_density_max_node": [float(v) for v in np.array(np.unravel_index(int(np.argmax(e)), e.shape)) / (m - 1.0)],
           "G_p": {str(int(p)): sol.stress_norm(p) for p in (4.0, 8.0, 16.0)}}
    print(json.dumps(out), flush=True)
    sol.operator.close()
    eq.backend.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--demo", action="store_true", help="run the L-bracket and add its figures to the file")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/stress)")
    ap.add_argument("--no-write", action="store_true", help="print only")
    a = ap.parse_args()
    import lsm_amd as lsm
    cases = [run(lsm, name, a.reps) for name in a.cases]
    dm = demo(lsm) if a.demo else None
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        for r in cases:
            for key in ("strain", "stress", "von_mises", "norm", "load", "sensitivity"):
                r[key]["frac_of_copy"] = round(r[key]["model_gbs"] / (copy_tbs * 1e3), 3)
    doc = {"cmd": "python tools/stress_bench.py --reps %d%s" % (a.reps, " --demo" if a.demo else ""), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "rtol": RTOL, "contrast": 1e-3, "nu": 0.3, "p": P, "cases": cases}
    if dm:
        doc["demo"] = dm
    os.makedirs(a.out, exist_ok=True)
    json.dump(doc, open(os.path.join(a.out, "stress_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
