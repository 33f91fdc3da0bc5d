#!/usr/bin/env python
"""Multi-load elasticity on the device: writes profiles/multiload/multiload_bench.json (and prints one JSON line per measurement).

The workload is tools/elastic_bench.py's: a plate (block) with two holes, ersatz contrast 1e-3, ν = 0.3, clamped on x = 0, fp64, mg,
rtol 1e-8, from a zero guess — with K ∈ {2, 4, 8} uniform tractions of different directions on the face x = 1.
  batch vs loop   one solve_many of K columns against the K solve calls of the same operator, in one process, alternating, --reps times
                  each after a warm-up that keeps the device busy for at least 50 ms; the host clock runs around work that ends in a
                  synchronise.  Medians, min and max, Σ iterations, ms per column-iteration, ratio = loop / batch.
  energy          energy_density(weights) of K = 4 against four energy_density() calls and their torch combination, and against the
                  copy yardstick (`--copy-tbs`, what tools/copy_bw reaches) with the bytes model K·N doubles read and one written per node.
  --single NAME   the single-solve path alone (ms per solve of ElasticityOperator.solve), one JSON line: run it alternately with
                  LSM_AMD_LIB pointing at the parent commit's library and without, to show that the single solve did not move.  A
                  library from before this tool has no batched entry points: --single leaves them out of the symbol check.
  --trace NAME K  one batched solve and the K single ones, for a run of its own under `rocprofv3 --kernel-trace`: the gaps between
                  the kernels of an iteration are read from the trace.
  --demo          a 2-D force inverter at 128×64: the input load and the output adjoint (homogeneous=True) as two columns, the speed
                  is mutual_energy_density(0, 1), a few steps; prints the output displacement cross_compliance(1, 0) per step (it should fall)."""
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

OUT = os.path.join(ROOT, "profiles", "multiload")
SIZES = {"256x256": (256, 256), "512x512": (512, 512), "1024x1024": (1024, 1024), "2048x2048": (2048, 2048), "32c": (32, 32, 32), "64c": (64, 64, 64),
         "128c": (128, 128, 128)}
RTOL = 1e-8
NEW = ("lsm_elastic_solve_many", "lsm_elastic_energy_many", "lsm_elastic_energy_mutual")


def loads(b, n, K):
    """K tractions on the face x = 1, each its own direction, as flat device arrays (component-major)"""
    t = b.torch
    N = len(n)
    nn = int(np.prod(n))
    face = t.arange(n[0] - 1, nn, n[0], device=b.device)
    out = []
    for k in range(K):
        ang = np.pi * (k + 1) / (K + 1)
        d = [np.cos(ang), -np.sin(ang)] + ([0.3 * np.cos(2.0 * ang)] if N > 2 else [])
        f = t.zeros(N * nn, dtype=t.float64, device=b.device)
        for i in range(N):
            f[i * nn + face] = 2.0 * (n[0] - 1) * d[i]
        out.append(f)
    return out


def spread(ts):
    return {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def timed(b, fn):
    b.sync()
    t = time.perf_counter()
    r = fn()
    b.sync()
    return (time.perf_counter() - t) * 1e3, r


def warm(b, fn, ms=50.0):
    spent = 0.0
    while spent < ms:
        spent += timed(b, fn)[0]


def run(lsm, name, Ks, reps):
    n = SIZES[name]
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond="mg")
    kw = dict(rtol=RTOL, max_iters=200000)
    out = []
    for K in Ks:
        fs = loads(b, n, K)
        loop = lambda: [op.solve(f, **kw) for f in fs]
        batch = lambda: op.solve_many(fs, **kw)
        warm(b, loop)
        warm(b, batch)
        tl, tb = [], []
        for _ in range(reps):
            ms, single = timed(b, loop)
            tl.append(ms)
            ms, many = timed(b, batch)
            tb.append(ms)
        its = tuple(s.iterations for s in single)
        assert its == many.iterations, (its, many.iterations)
        r = {"case": name, "n": list(n), "K": K, "reps": reps, "iterations": list(its), "sum_iterations": sum(its), "levels": op.levels,
             "loop": spread(tl), "batch": spread(tb)}
        r["loop"]["ms_per_column_iteration"] = round(r["loop"]["ms"] / sum(its), 4)
        r["batch"]["ms_per_column_iteration"] = round(r["batch"]["ms"] / sum(its), 4)
        r["ratio_loop_over_batch"] = round(r["loop"]["ms"] / r["batch"]["ms"], 3)
        print(json.dumps(r), flush=True)
        out.append(r)
        del single, many
    op.close()
    eq.backend.close()
    return out


def run_energy(lsm, name, copy_tbs, reps):
    n = SIZES[name]
    N, K = len(n), 4
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond="mg")
    many = op.solve_many(loads(b, n, K), rtol=RTOL, max_iters=200000)
    w = (0.4, 0.3, 0.2, 0.1)

    def four():
        e = [s.energy_density() for s in many]
        acc = b.torch.zeros_like(e[0].buf)
        for wk, ek in zip(w, e):
            acc = acc + wk * ek.buf
        return acc

    one = lambda: many.energy_density(w)
    warm(b, four)
    warm(b, one)
    t4, t1 = [], []
    for _ in range(reps * 4):
        t4.append(timed(b, four)[0])
        t1.append(timed(b, one)[0])
    nbytes = (K * N + 1) * 8 * int(np.prod(n))
    r = {"case": name, "K": K, "four_calls_and_torch": spread(t4), "one_pass": spread(t1), "model_bytes": nbytes,
         "one_pass_tbs": round(nbytes / (statistics.median(t1) * 1e-3) / 1e12, 3), "copy_tbs_8B_per_lane": copy_tbs}
    if copy_tbs:
        r["frac_of_copy"] = round(r["one_pass_tbs"] / copy_tbs, 3)
    print(json.dumps(r), flush=True)
    op.close()
    eq.backend.close()
    return r


def single(name, reps):
    import lsm_amd as lsm
    if os.environ.get("LSM_AMD_LIB"):      # before the library is first loaded
        lsm._lib._SIGS[:] = [s for s in lsm._lib._SIGS if s[0] not in NEW]
    n = SIZES[name]
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond="mg")
    f = loads(b, n, 1)[0]
    kw = dict(rtol=RTOL, max_iters=200000)
    warm(b, lambda: op.solve(f, **kw))
    ts = []
    for _ in range(reps):
        ms, sol = timed(b, lambda: op.solve(f, **kw))
        ts.append(ms)
    print(json.dumps({"case": name, "lib": os.environ.get("LSM_AMD_LIB") or "tree", "iterations": sol.iterations, **spread(ts)}), flush=True)
    op.close()


def trace(lsm, name, K):
    n = SIZES[name]
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond="mg")
    fs = loads(b, n, K)
    kw = dict(rtol=RTOL, max_iters=200000)
    for _ in range(2):
        [op.solve(f, **kw) for f in fs]
        op.solve_many(fs, **kw)
    b.sync()
    op.close()


def demo(lsm, steps):
    n = (128, 64)
    grid = lsm.CartesianGrid((0.0, 0.0), (2.0, 1.0), n)
    x, y = np.meshgrid(np.linspace(0, 2, n[0]), np.linspace(0, 1, n[1]), indexing="ij")
    phi0 = np.asfortranarray(0.06 - np.abs(np.cos(3.0 * np.pi * x) * np.cos(3.0 * np.pi * y)) * 0.2)      # a perforated plate, material where ϕ < 0
    f_in, f_out = np.zeros((2,) + n), np.zeros((2,) + n)
    mid = slice(n[1] // 2 - 3, n[1] // 2 + 4)
    f_in[0][0, mid] = 1.0          # the input pushes in +x at the middle of the left face
    f_out[0][-1, mid] = 1.0        # the objective J = l·u: the displacement in +x at the middle of the right face, to be lowered (inverted)
    mask = np.zeros(n + (2,), dtype=bool)
    mask[0, :4, :] = mask[0, -4:, :] = True      # clamped near the left corners
    state = {}

    def update(coeff, phi, t):
        many = lsm.elasticity_solve_many(phi, [f_in, f_out], homogeneous=(False, True), dirichlet=(mask, 0.0), rtol=1e-8)
        state["out"] = many.cross_compliance(1, 0)
        m = many.mutual_energy_density(0, 1)
        # dJ/dE_C = −∏h·u_C·K0 v_C: material added where m > 0 lowers J, so the boundary moves outwards with the speed m
        coeff.set_values(m)
        many.operator.close()

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update), lsm.EikonalReinitializationTerm()),
                              ic=lsm.MeshField(phi0, grid), bc=lsm.NeumannBC(), integrator=lsm.RK2())
    t = 0.0
    for k in range(steps):
        dt = 0.5 * eq.compute_cfl(t)
        t += dt
        lsm.integrate_(eq, t)
        print(json.dumps({"step": k, "t": t, "output_displacement": state["out"], "volume": lsm.volume(eq)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--K", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--energy", nargs="*", default=["1024x1024", "128c"], choices=list(SIZES), help="the cases of the energy_density(weights) measurement")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--single", metavar="NAME", choices=list(SIZES), help="time the single solve alone and exit")
    ap.add_argument("--trace", nargs=2, metavar=("NAME", "K"), help="one batched solve and the K single ones, for a kernel trace")
    ap.add_argument("--demo", action="store_true", help="the force inverter")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if a.single:
        single(a.single, a.reps)
        return
    import lsm_amd as lsm
    if a.trace:
        trace(lsm, a.trace[0], int(a.trace[1]))
        return
    if a.demo:
        demo(lsm, a.steps)
        return
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "multiload_bench.json")
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    doc = {"cmd": "python tools/multiload_bench.py --reps %d --cases %s --K %s" % (a.reps, " ".join(a.cases), " ".join(map(str, a.K))),
           "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL, "precond": "mg", "copy_tbs_8B_per_lane": copy_tbs, "solves": [], "energy": []}
    for name in a.cases:        # the file is rewritten after every case: a long one may be cut short
        doc["solves"] += run(lsm, name, a.K, a.reps)
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)
    for name in a.energy:
        doc["energy"].append(run_energy(lsm, name, copy_tbs, a.reps))
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
