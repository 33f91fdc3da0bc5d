#!/usr/bin/env python
"""SemiImplicitI2OE on the device: one JSON line per case.

  ms_per_step      wall time of integrate_ per step (the host loop, compute_cfl and the solve), median of --reps runs
  iters_per_step   BiCGSTAB iterations per step
  gbs, hbm_frac    effective bandwidth of the solve under the traffic model below, and its fraction of the 8 TB/s HBM peak
  t_i2oe_ms        time to tf with SemiImplicitI2OE(cfl) ...
  t_rk3_ms         ... and with RK3() + Upwind() on the same equation (cfl 0.5), and the ratio of the two

Traffic model (fp64, compact vectors, each array moved once per kernel, neighbour reads from cache):
  per iteration  K1 reads N face arrays + r, p, v, r̂ and writes p', v'; K2 reads N face arrays + r, v' and writes s, t;
                 K3 reads x, p', s, t, r̂ and writes x, r            → (2N + 17) · 8 bytes per node
  per step       face assembly (N arrays written), rhs/init (ϕ read, N face arrays, 5 vectors written), store (x read,
                 ϕ written)                                          → (2N + 8) · 8 bytes per node (+ velocity reads)
Cases: the docs' 64² dumbbell (one revolution), a 2048² rotation and the 256³ vortex (vortex_deformation) at cfl 2 and 4.
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lsm_amd as lsm

HBM_PEAK = 8.0e12


def dumbbell(grid):
    disk = lambda c: lsm.MeshField(lambda x: np.hypot(x[0] - c[0], x[1] - c[1]) - 0.25, grid).vals
    bar = lsm.MeshField(lambda x: np.maximum(np.abs(x[0]) - 0.5, np.abs(x[1]) - 0.1), grid).vals
    return lsm.MeshField(np.minimum(np.minimum(disk((-0.5, 0.0)), disk((0.5, 0.0))), bar), grid)


def case(name):
    """(grid, ic, velocity, bc, tf in units of I2OE steps at cfl 2 or None for a full revolution)"""
    if name == "dumbbell64":
        g = lsm.CartesianGrid((-1, -1), (1, 1), (64, 64))
        return g, dumbbell(g), lsm.RigidRotation(), lsm.NeumannBC(), None
    if name == "rotation2048":
        g = lsm.CartesianGrid((-1, -1), (1, 1), (2048, 2048))
        return g, lsm.MeshField(lambda x: np.hypot(x[0] - 0.4, x[1]) - 0.3, g), lsm.RigidRotation(), lsm.NeumannBC(), 20
    g = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), (256, 256, 256))
    ic = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.35) ** 2 + (x[1] - 0.35) ** 2 + (x[2] - 0.35) ** 2) - 0.15, g)
    return g, ic, lsm.vortex_deformation(g), lsm.NeumannBC(), 10


def run(grid, ic, vel, bc, integ, scheme, tf, reps):
    times, steps, iters = [], 0, 0
    for _ in range(reps + 1):   # the first run warms up (handle, workspace, kernels) and is not counted
        eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel, scheme), ic=ic, bc=bc, integrator=integ)
        n = [0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lsm.integrate_(eq, tf, posthook=lambda e: n.__setitem__(0, n[0] + 1))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        steps, iters = n[0], getattr(eq, "i2oe_iters", 0)
        eq.backend.close()
    return float(np.median(times[1:])), steps, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="dumbbell64,rotation2048,vortex256")
    ap.add_argument("--cfl", default="2,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-rk3", action="store_true", help="skip the RK3 + Upwind comparison")
    args = ap.parse_args()
    for name in args.cases.split(","):
        grid, ic, vel, bc, nsteps = case(name)
        N = grid.ndim
        nn = int(np.prod(grid.n))
        h = grid.meshsize()
        for cfl in (float(c) for c in args.cfl.split(",")):
            if name == "dumbbell64" and cfl != 2.0:
                continue
            if nsteps is None:
                tf = 2 * math.pi
            else:   # nsteps I2OE steps at cfl 2 (the CFL of the initial velocity)
                eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel, lsm.Upwind()), ic=ic, bc=bc, integrator=lsm.RK3())
                tf = nsteps * 2.0 * eq.compute_cfl()
                eq.backend.close()
            ms, steps, iters = run(grid, ic, vel, bc, lsm.SemiImplicitI2OE(cfl=cfl), lsm.Upwind(), tf, args.reps)
            ips = iters / steps
            bytes_step = (ips * (2 * N + 17) + (2 * N + 8)) * 8 * nn
            rec = {"case": name, "n": list(grid.n), "cfl": cfl, "tf": tf, "steps": steps, "ms_per_step": round(ms / steps, 4),
                   "iters_per_step": round(ips, 2), "bytes_per_node_iter": (2 * N + 17) * 8,
                   "gbs": round(bytes_step / (ms / steps * 1e-3) / 1e9, 1), "t_i2oe_ms": round(ms, 2)}
            rec["hbm_frac"] = round(rec["gbs"] * 1e9 / HBM_PEAK, 3)
            if not args.no_rk3:
                ms3, steps3, _ = run(grid, ic, vel, bc, lsm.RK3(), lsm.Upwind(), tf, max(1, args.reps // 2))
                rec.update({"rk3_steps": steps3, "t_rk3_ms": round(ms3, 2), "rk3_over_i2oe": round(ms3 / ms, 3)})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
