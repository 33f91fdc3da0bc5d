#!/usr/bin/env python
"""The topological derivative and the nucleation step on the device: writes profiles/topology/topo_bench.json (and prints one JSON
line per case).

The workload, fp64, at 2048² and 256³: elastic_bench's block with two holes as a signed distance, a smooth displacement given through
with_displacement (the T field needs no solve); per call (median, min, max of --reps after a warm-up, the stream synchronised around
each):
  topo          lsm_elastic_topo into a field that exists: the cell pass into scratch and the node gather
  search_w2     lsm_nucleate_create + read + destroy with t = T, threshold = the median of T, clearance 2h, spacing 1.5h (w = 2)
  search_w16    the same with spacing 15.5h (w = 16)
  punch         lsm_nucleate_punch of search_w16's centres with radius 4h into a copy of ϕ (the copy is not timed)
  model_gbs     MODEL bytes / ms, against `--copy-tbs` (tools/copy_bw's 8-bytes-per-lane copy of the same run, read + write, when the
                option is absent and the program is built).  The model counts every array once: topo reads the N fields of u and the
                cell moduli, writes and reads the cell array, writes the node field (8 bytes an entry); the search reads t and ϕ,
                writes and reads a 12-byte key per node and pass, and reads the last pass's keys twice (count, write); the punch
                clears and reads 8 bytes per node and reads ϕ.
--demo: a 2-D cantilever (2 × 1, clamped on x = 0, a downward traction on the middle fifth of x = 2) that starts from the FULL box:
the descent of compliance + ℓ·volume by NormalMotionTerm with the speed e − ℓ, and every --every steps nucleate_ with t = T,
threshold = ℓ (a hole pays where T < ℓ), then reinitialize_; compliance, volume and components(side="outside") per iteration, into
the same file."""
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

from elastic_bench import copy_yardstick, field, two_holes

OUT = os.path.join(ROOT, "profiles", "topology")
SIZES = {"2048x2048": (2048, 2048), "256c": (256, 256, 256)}
KEYS = ("topo", "search_w2", "search_w16", "punch")


def model_bytes(N, n):
    nodes, cells = float(np.prod(n)), float(np.prod([m - 1 for m in n]))
    search = (16.0 + 12.0) + (N - 1) * 24.0 + 2 * 12.0
    return {"topo": 8.0 * ((N + 1) * nodes + 3 * cells), "search_w2": search * nodes, "search_w16": search * nodes, "punch": 24.0 * nodes}


def timed(b, reps, call, before=None):
    if before:
        before()
    call()
    ts = []
    for _ in range(reps):
        if before:
            before()
        b.sync()
        t = time.perf_counter()
        call()
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"ms_per_call": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def smooth_u(n):
    ax = [np.linspace(0.0, 1.0, m) for m in n]
    x = np.meshgrid(*ax, indexing="ij", sparse=True)
    return [np.asfortranarray(np.sin(3.0 * x[i] + 0.7 * i) * np.cos(2.0 * x[(i + 1) % len(n)]) + np.zeros(n)) for i in range(len(n))]


def run(lsm, name, reps):
    n = SIZES[name]
    N = len(n)
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    h = float(min(phi.mesh.meshsize()))
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    sol = op.with_displacement(smooth_u(n))
    hd, ub = op._handle(), [c.buf for c in sol.u]
    T = sol.topological_derivative()
    threshold = float(np.median(T.values()))
    res = {"case": name, "n": list(n), "nodes": int(np.prod(n)), "reps": reps, "threshold": threshold}
    find = lambda w: b.nucleate_find(phi.buf, T.buf, threshold, 0.0, 2.0 * h, (w - 0.5) * h)
    idx = {w: find(w)[0] for w in (2, 16)}
    res["centres"] = {"w2": int(idx[2].size), "w16": int(idx[16].size)}
    work = phi.copy()
    calls = {"topo": (lambda: b.elastic_topo(hd, ub, T.buf), None), "search_w2": (lambda: find(2), None), "search_w16": (lambda: find(16), None),
             "punch": (lambda: b.nucleate_punch(work.buf, idx[16], 0.0, 4.0 * h), lambda: work.copy_(phi))}
    mb = model_bytes(N, n)
    for key, (call, before) in calls.items():
        r = timed(b, reps, call, before)
        r["model_bytes"] = mb[key]
        r["model_gbs"] = round(mb[key] / (r["ms_per_call"] * 1e-3) / 1e9, 1)
        res[key] = r
    res["punch"]["changed"] = b.nucleate_punch(work.copy_(phi).buf, idx[16], 0.0, 4.0 * h)
    print(json.dumps(res), flush=True)
    del sol
    op.close()
    eq.backend.close()
    return res


def demo(lsm, m=65, steps=24, every=6, holes=4):
    n, hc = (2 * m - 1, m), (2.0, 1.0)
    grid = lsm.CartesianGrid((0.0, 0.0), hc, n)
    h = float(min(grid.meshsize()))
    ax = [np.linspace(0.0, c, k) for c, k in zip(hc, n)]
    x, y = np.meshgrid(*ax, indexing="ij")
    full = np.asfortranarray(-(0.5 * h + np.minimum.reduce([x, y, hc[0] - x, hc[1] - y])))      # the signed distance of a box half a cell larger
    f = np.zeros((2,) + n)
    f[1][(x == hc[0]) & (np.abs(y - 0.5) <= 0.1)] = -2.0 / h
    clamp = lsm.face_mask(grid, 0, 0)
    state = {}

    def solve(phi, want_T=False):
        sol = lsm.elasticity_solve(phi, f, dirichlet=(clamp, 0.0), rtol=1e-8, max_iters=20000)
        state["compliance"], state["iterations"] = sol.compliance(), sol.iterations
        out = sol.energy_density(), (sol.topological_derivative() if want_T else None)
        sol.operator.close()
        return out

    def update(coeff, phi, t):
        e, _ = solve(phi)
        e.buf.sub_(state["ell"])          # the speed e − ℓ, on the device
        coeff.set_values(e)

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(full, grid), bc=lsm.NeumannBC(),
                              integrator=lsm.RK3())
    phi = eq.current_state()
    e, T = solve(phi, True)
    state["ell"] = ell = float(np.median(T.values()))
    tau = h / float(np.abs(e.values() - ell).max())
    hist = []
    for k in range(steps):
        _, T = solve(phi, True)
        row = {"step": k, "compliance": state["compliance"], "volume": lsm.volume(eq), "outside_components": lsm.components(phi, side="outside").count,
               "pcg_iterations": state["iterations"]}
        if k % every == 0:
            nuc = lsm.nucleate_(phi, T, threshold=ell, radius=3.0 * h, clearance=5.0 * h, max_holes=holes)
            row["nucleated"], row["found"], row["changed"] = len(nuc), nuc.found, nuc.changed
            if len(nuc):
                lsm.reinitialize_(phi)
        row["objective"] = row["compliance"] + ell * row["volume"]
        hist.append(row)
        print(json.dumps(row), flush=True)
        if lsm.components(phi, side="outside").count:      # a full box has no interface to move
            lsm.integrate_(eq, eq.current_time() + tau)
    eq.backend.close()
    return {"grid": list(n), "ell": ell, "radius_h": 3.0, "clearance_h": 5.0, "max_holes": holes, "nucleate_every": every,
            "outer_step": "one cell at the first step's largest speed", "history": hist}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", nargs="*", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--demo", action="store_true", help="run the cantilever descent from the full box and add its history to the file")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/topology)")
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
            for key in KEYS:
                r[key]["frac_of_copy"] = round(r[key]["model_gbs"] / (copy_tbs * 1e3), 3)
    doc = {"cmd": "python tools/topo_bench.py --reps %d%s" % (a.reps, " --demo" if a.demo else ""), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "cases": cases}
    if dm:
        doc["demo"] = dm
    os.makedirs(a.out, exist_ok=True)
    json.dump(doc, open(os.path.join(a.out, "topo_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
