#!/usr/bin/env python
"""extend_from_interface_ on the device: writes profiles/extend/extend_bench.json (and prints one JSON line per case).

The workload: the sphere of radius 0.5 in [−1, 1]³ at 96³ and 256³; ϕ = |x|² − 0.25 redistanced by eikonal_ (crossing seed), the
fields the components of x/|x| and |x| itself, extended from eikonal_'s seeding set (the crossing seed) over the whole grid.
  ms_per_call       wall time of one synchronous lsm_extend (init kernel and its host read, the tile launches with one host read of
                    the list length each, the check and its host read, the final pass): median, min and max of --reps calls after
                    the warm-up calls (at least two, and at least 100 ms of them); the fields are restored from copies before
                    each call, outside the timed window.  K1: one field; K4: four fields in one call; 4xK1: the same four fields
                    in four calls, timed as one; the three and extend_along_normals_ are taken in turn, call by call
  iterations        outer iterations (launches of the tile kernel); visits: tiles visited over all of them — next to eikonal_'s
                    own on the same input
  normals           extend_along_normals_ on the first field with the nb_iters that carries information as far, n/(2·cfl) sweeps
                    at cfl = 0.45 (frozen: its own band rule)
  max_err           max |F − x/|x|| over |x| > 0.15, first component

Kernel shares: run the same command with --no-write --only N under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`,
then `--stats DIR` adds every ex_* / ek_* kernel's dispatches and total time, and the init and final passes' rates under their
traffic models (init: 8 bytes of ϕ read, 8 of g, 1 of the fixed byte and 8·K of working copies written per node; final: 8·K read
and 8·K written) against `--copy-tbs`, what tools/copy_bw reaches with 8 bytes per lane (read + write; the tool is run when the
option is absent and the program is built).

--demo: the thermal-compliance descent of tools/elliptic_bench.py --demo with the speed e − ℓ extended from the solid
(frozen="inside") before each advection, next to the same descent without the extension."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

OUT = os.path.join(ROOT, "profiles", "extend")
CFL = 0.45
INF = float("inf")


def fields(lsm, n):
    """(the equation, ϕ redistanced by eikonal_, eikonal_'s stats, four device fields, device copies of them, x/|x| on the host, r)"""
    grid = lsm.CartesianGrid((-1.0,) * 3, (1.0,) * 3, (n,) * 3)
    ax = np.linspace(-1.0, 1.0, n)
    X = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    r = np.sqrt(X[0] ** 2 + X[1] ** 2 + X[2] ** 2) + np.zeros((n,) * 3)
    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=lsm.MeshField(np.asfortranarray(r * r - 0.25), grid), bc=lsm.ExtrapolationBC(2))
    phi = eq.current_state()
    ek = phi.backend.eikonal(phi.buf, None, 0.0, INF, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        host = [np.asfortranarray(np.where(r > 0, X[d] / r, 0.0)) for d in range(3)] + [np.asfortranarray(r)]
    F = [phi.copy().copy_(f) for f in host]
    keep = [f.buf.clone() for f in F]
    return eq, phi, ek, F, keep, host[0], r


def interleaved(b, F, keep, reps, calls):
    """calls: name → the call; every round restores the fields and runs each once, in turn.  Returns name → [ms]"""
    def restore():
        for f, k in zip(F, keep):
            f.buf.copy_(k)
    ts = {k: [] for k in calls}
    warm, t_warm = 0, time.perf_counter()
    while warm < 2 or time.perf_counter() - t_warm < 0.1:
        for call in calls.values():
            restore()
            call()
        b.sync()
        warm += 1
    for _ in range(reps):
        for k, call in calls.items():
            restore()
            b.sync()
            t = time.perf_counter()
            call()
            b.sync()
            ts[k].append((time.perf_counter() - t) * 1e3)
    restore()
    return ts


def summary(ts):
    return {"ms_per_call": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def run(lsm, n, reps, with_normals=True):
    eq, phi, ek, F, keep, want, r = fields(lsm, n)
    b = phi.backend
    stats = {}
    bufs = [f.buf for f in F]

    def four():
        for x in bufs:
            stats["4xK1"] = b.extend([x], phi.buf)
    calls = {"K1": lambda: stats.__setitem__("K1", b.extend(bufs[:1], phi.buf)),
             "K4": lambda: stats.__setitem__("K4", b.extend(bufs, phi.buf)),
             "4xK1": four}
    nb_iters = int(round(n / (2 * CFL)))
    if with_normals:
        calls["normals"] = lambda: lsm.extend_along_normals_(F[0], phi, nb_iters=nb_iters, cfl=CFL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts = interleaved(b, F, keep, reps, calls)
    out = []
    far = r > 0.15
    for k, call in calls.items():
        for f, kp in zip(F, keep):
            f.buf.copy_(kp)
        call()
        res = {"case": f"sphere{n}", "n": n, "what": k, "reps": reps, **summary(ts[k]), "max_err": round(float(np.abs(F[0].values() - want)[far].max()), 6)}
        if k in stats:
            frozen, iters, visits, orphans, filled = stats[k]
            tiles = ((n + 7) // 8) ** 3
            res.update({"frozen_nodes": frozen, "iterations": iters, "visits": visits, "visits_per_tile": round(visits / tiles, 3), "orphans": orphans,
                        "tiles": tiles, "nodes_per_s": round(n ** 3 / (res["ms_per_call"] * 1e-3)),
                        "eikonal_iterations": ek[1], "eikonal_visits": ek[2], "eikonal_visits_per_tile": round(ek[2] / tiles, 3)})
        else:
            res["nb_iters"] = nb_iters
        print(json.dumps(res), flush=True)
        out.append(res)
    eq.backend.close()
    return out


def demo(lsm, m=129, steps=12, reinit_every=4):
    """tools/elliptic_bench.py's descent, once with the raw speed e − ℓ and once with it extended from the solid"""
    import elliptic_bench as EB
    n = (m, m)
    eq0, phi0 = EB.field(lsm, n, EB.two_holes(n))
    grid = phi0.mesh
    h = min(grid.meshsize())
    patch = lsm.face_mask(grid, 0, 0)
    patch[:, : m // 3] = False
    patch[:, 2 * m // 3:] = False
    state = {}

    def solve(phi):
        sol = lsm.elliptic_solve(phi, 1.0, dirichlet=(patch, 0.0), rtol=EB.RTOL)
        e = sol.energy_density()
        state["compliance"], state["iterations"] = sol.compliance(), sol.iterations
        sol.operator.close()
        return e

    e = solve(phi0)
    ell = float(e.values()[phi0.values() < 0].mean())
    vmax = float(np.abs(e.values() - ell).max())
    eq0.backend.close()
    out = {"grid": list(n), "ell": ell, "outer_step": "one cell at the first step's largest speed", "reinitialize_every": reinit_every}
    for name, extended in (("raw_speed", False), ("extended_from_the_solid", True)):
        def update(coeff, phi, t):
            e = solve(phi)
            e.buf.sub_(ell)                   # the speed e − ℓ, on the device
            if extended:
                state["extend"] = phi.backend.extend([e.buf], phi.buf, "inside")
            coeff.set_values(e)

        eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update),), ic=lsm.MeshField(EB.two_holes(n), grid),
                                  bc=lsm.NeumannBC(), integrator=lsm.RK3())
        hist, tau = [], h / vmax
        for k in range(steps):
            solve(eq.current_state())
            hist.append({"step": k, "compliance": state["compliance"], "volume": lsm.volume(eq), "pcg_iterations": state["iterations"]})
            hist[-1]["objective"] = hist[-1]["compliance"] + ell * hist[-1]["volume"]
            if "extend" in state:
                hist[-1]["extend_stats"] = list(state["extend"])
            print(json.dumps({"run": name, **hist[-1]}), flush=True)
            lsm.integrate_(eq, eq.current_time() + tau)
            if (k + 1) % reinit_every == 0:
                lsm.reinitialize_(eq.current_state())
        eq.backend.close()
        state.pop("extend", None)
        out[name] = hist
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
        m = re.search(r"\b(ex|ek)_\w+_kernel(<[\w:, ]+>)?", r["Name"].split("(")[0])
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 256])
    ap.add_argument("--only", type=int, help="one size, K = 4 calls only (the run under the profiler: every dispatch is that grid's and that K's)")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--stats-n", type=int, default=256, help="the grid the traced run used (--only)")
    ap.add_argument("--demo", action="store_true", help="run the thermal-compliance descents and add their histories to the file")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/extend)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "extend_bench.json")
    if a.stats:
        doc = json.load(open(path))
        ks = kernel_stats(a.stats)
        K, nodes = 4, a.stats_n ** 3
        doc["kernel_trace"] = {"cmd": f"rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/extend_bench.py --no-write --only {a.stats_n}; "
                                      f"python tools/extend_bench.py --stats <dir> --stats-n {a.stats_n}",
                               "n": a.stats_n, "K": K, "note": "K = 4 calls, warm-up calls and the one eikonal_ solve included (traced, so slower than the plain run)",
                               "kernels": ks}
        for key, kname, nbytes in (("init", "ex_init_kernel", 8 + 8 + 1 + 8 * K), ("final", "ex_write_kernel", 16 * K)):
            hit = [v for k, v in ks.items() if k.startswith(kname)]
            if hit:
                gbs = nbytes * nodes / (hit[0]["us_per_dispatch"] * 1e-6) / 1e9
                doc["kernel_trace"][f"{key}_model_bytes_per_node"] = nbytes
                doc["kernel_trace"][f"{key}_model_gbs"] = round(gbs, 1)
                if doc.get("copy_tbs_8B_per_lane"):
                    doc["kernel_trace"][f"{key}_frac_of_copy"] = round(gbs / (doc["copy_tbs_8B_per_lane"] * 1e3), 3)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        eq, phi, ek, F, keep, want, r = fields(lsm, a.only)
        b = phi.backend
        ts = interleaved(b, F, keep, a.reps, {"K4": lambda: b.extend([f.buf for f in F], phi.buf)})
        print(json.dumps({"n": a.only, "what": "K4", **summary(ts["K4"])}))
        eq.backend.close()
        return
    cases = []
    for n in a.sizes:
        cases += run(lsm, n, a.reps)
    dm = demo(lsm) if a.demo else None
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    doc = {"cmd": "python tools/extend_bench.py --reps %d%s" % (a.reps, " --demo" if a.demo else ""), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "tile": [8, 8, 8], "passes_per_visit": 8, "fields_per_workgroup": 4, "cases": cases}
    if dm:
        doc["demo"] = dm
    json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
