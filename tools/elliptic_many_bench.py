#!/usr/bin/env python
"""Multi-source elliptic solves on the device: writes profiles/elliptic_many/elliptic_many_bench.json (and prints one JSON line per
measurement).  DESIGN.md §7.27.

The workload is tools/elliptic_bench.py's plate (block) with two holes, ersatz contrast 1e-3, u = 0 on x = 0, fp64, mg, rtol 1e-8,
from a zero guess — with K ∈ {2, 4, 8} sources: a uniform one and K − 1 Gaussian heat spots at different places.
  batch vs loop   one solve_many of K columns against the K solve calls of the same operator, in one process, alternating, --reps times
                  each after a warm-up that keeps the device busy for at least 50 ms; the host clock runs around work that ends in a
                  synchronise.  Medians, min and max, Σ iterations, ms per column-iteration, ratio = loop / batch.
  energy          energy_density(weights) of K = 4 against four energy_density() calls and their torch combination.
  --single LIB    the single solve of this tree against the library LIB of the parent commit (through LSM_AMD_LIB), alternating in fresh
                  processes at 512² and 128³, --rounds times each: medians of --reps solves per process.  Writes single_ab.json.
  --k1 LIB        the K1 A/B of §7.27: LIB is a library built from the tree with profiles/elliptic_many/k1_ab.patch applied, which
                  holds both K1 kernels of the batch (the node-owned one that the tree keeps and the z-column one that it dropped) and a
                  probe that times them per launch on the batch workspace, interleaved in one process (events around --launches
                  launches, --rounds rounds), at 2048² and 128³ for K = 4 and 8.  Runs in a fresh process with LSM_AMD_LIB = LIB.
                  Writes k1_ab.json.
  --demo          a sensor-temperature descent at 128×64: the heat load and the sensor functional l (homogeneous=True) as the two
                  columns of one batch, the speed is mutual_energy_density(0, 1), a few steps; prints l·u per step (it should fall)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from elastic_bench import field, two_holes

OUT = os.path.join(ROOT, "profiles", "elliptic_many")
SIZES = {"256x256": (256, 256), "512x512": (512, 512), "1024x1024": (1024, 1024), "2048x2048": (2048, 2048), "32c": (32, 32, 32), "64c": (64, 64, 64),
         "128c": (128, 128, 128)}
RTOL = 1e-8
NEW = ("lsm_elliptic_solve_many", "lsm_elliptic_energy_many", "lsm_elliptic_energy_mutual")


def sources(b, n, K):
    """K sources as flat float64 device arrays: the uniform one, then Gaussian spots of width 0.08 on a circle around the centre"""
    t = b.torch
    ax = [t.linspace(0.0, 1.0, m, dtype=t.float64, device=b.device) for m in n]
    out = [t.ones(int(np.prod(n)), dtype=t.float64, device=b.device)]
    for k in range(1, K):
        ang = 2.0 * np.pi * k / K
        c = [0.5 + 0.3 * np.cos(ang), 0.5 + 0.3 * np.sin(ang), 0.5][:len(n)]
        g = [t.exp(-((x - ci) / 0.08) ** 2) for x, ci in zip(ax, c)]
        f = g[0]
        for d in range(1, len(n)):      # axis 0 fastest
            f = (g[d].reshape(-1, 1) * f.reshape(1, -1)).reshape(-1)
        out.append(100.0 * f.contiguous())
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


def operator(lsm, n):
    eq, phi = field(lsm, n, two_holes(n))
    return eq, phi.backend, lsm.EllipticOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0), precond="mg")


def run(lsm, name, Ks, reps):
    n = SIZES[name]
    eq, b, op = operator(lsm, n)
    kw = dict(rtol=RTOL, max_iters=200000)
    out = []
    for K in Ks:
        fs = sources(b, n, K)
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


def run_energy(lsm, name, reps):
    n = SIZES[name]
    K = 4
    eq, b, op = operator(lsm, n)
    many = op.solve_many(sources(b, n, K), rtol=RTOL, max_iters=200000)
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
    nbytes = (K + 1) * 8 * int(np.prod(n))      # K doubles read and one written per node; the cells come on top
    r = {"case": name, "K": K, "four_calls_and_torch": spread(t4), "one_pass": spread(t1), "model_bytes": nbytes,
         "one_pass_tbs": round(nbytes / (statistics.median(t1) * 1e-3) / 1e12, 3)}
    print(json.dumps(r), flush=True)
    op.close()
    eq.backend.close()
    return r


def single_child(name, reps):
    import lsm_amd as lsm
    if os.environ.get("LSM_AMD_LIB"):      # a library from before this tool has no batched entry points; before the library is first loaded
        lsm._lib._SIGS[:] = [s for s in lsm._lib._SIGS if s[0] not in NEW]
    n = SIZES[name]
    eq, b, op = operator(lsm, n)
    f = sources(b, n, 1)[0]
    kw = dict(rtol=RTOL, max_iters=200000)
    warm(b, lambda: op.solve(f, **kw))
    ts = []
    for _ in range(reps):
        ms, sol = timed(b, lambda: op.solve(f, **kw))
        ts.append(ms)
    print(json.dumps({"case": name, "lib": "parent" if os.environ.get("LSM_AMD_LIB") else "tree", "iterations": sol.iterations, **spread(ts)}), flush=True)
    op.close()


def child(args, lib=None):
    """a fresh process of this tool, with LSM_AMD_LIB = lib or without it; its JSON lines"""
    env = dict(os.environ)
    env.pop("LSM_AMD_LIB", None)
    if lib:
        env["LSM_AMD_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (args, r.returncode, r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def single_ab(parent_lib, reps, rounds, out):
    doc = {"cmd": "python tools/elliptic_many_bench.py --single PARENT_LIB --reps %d --rounds %d" % (reps, rounds), "runs": []}
    for name in ("512x512", "128c"):
        for _ in range(rounds):
            for lib in (parent_lib, None):
                r = child(["--single-child", name, "--reps", str(reps)], lib)[0]
                print(json.dumps(r), flush=True)
                doc["runs"].append(r)
    json.dump(doc, open(os.path.join(out, "single_ab.json"), "w"), indent=1)


def k1_child(launches, rounds):
    import lsm_amd as lsm
    out = []
    for name in ("2048x2048", "128c"):
        n = SIZES[name]
        eq, b, op = operator(lsm, n)
        probe = b.lib.lsm_elliptic_k1_probe
        probe.restype, probe.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        for K in (4, 8):
            op.solve_many(sources(b, n, K), rtol=0.5, max_iters=200000)      # the workspace, with search directions that are not zero
            ms = (C.c_double * (2 * rounds))()
            code = probe(op._handle(), K, launches, rounds, ms)
            assert code == 0, code
            z, node = [ms[2 * r] for r in range(rounds)], [ms[2 * r + 1] for r in range(rounds)]
            r = {"case": name, "K": K, "launches": launches, "rounds": rounds, "z_column": spread(z), "node_owned": spread(node)}
            print(json.dumps(r), flush=True)
            out.append(r)
        op.close()
        eq.backend.close()
    return out


def demo(lsm, steps):
    n = (128, 64)
    grid = lsm.CartesianGrid((0.0, 0.0), (2.0, 1.0), n)
    x, y = np.meshgrid(np.linspace(0, 2, n[0]), np.linspace(0, 1, n[1]), indexing="ij")
    phi0 = np.asfortranarray(0.06 - np.abs(np.cos(3.0 * np.pi * x) * np.cos(3.0 * np.pi * y)) * 0.2)      # a perforated conductor, material where ϕ < 0
    heat = np.asfortranarray(np.exp(-((x - 1.5) ** 2 + (y - 0.5) ** 2) / 0.02))       # the load: a hot spot
    sensor = np.asfortranarray(np.exp(-((x - 1.0) ** 2 + (y - 0.75) ** 2) / 0.005))   # l: the temperature around a sensor, to be lowered
    sink = lsm.face_mask(grid, 0, 0)                                                  # u = 0 on x = 0
    state = {}

    def update(coeff, phi, t):
        many = lsm.elliptic_solve_many(phi, [heat, sensor], homogeneous=(False, True), dirichlet=(sink, 0.0), rtol=1e-8)
        state["J"] = many.cross_compliance(1, 0)
        # dJ/da_C = −∏h·(∇u·∇v)_C: conductor added where m = a∇u·∇v > 0 lowers J, so the boundary moves outwards with the speed m
        coeff.set_values(many.mutual_energy_density(0, 1))
        many.operator.close()

    eq = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(lsm.MeshField(np.zeros(n), grid), update), lsm.EikonalReinitializationTerm()),
                              ic=lsm.MeshField(phi0, grid), bc=lsm.NeumannBC(), integrator=lsm.RK2())
    t = 0.0
    for k in range(steps):
        dt = 0.5 * eq.compute_cfl(t)
        t += dt
        lsm.integrate_(eq, t)
        print(json.dumps({"step": k, "t": t, "sensor_temperature": state["J"], "volume": lsm.volume(eq)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--K", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--energy", nargs="*", default=["1024x1024", "128c"], choices=list(SIZES), help="the cases of the energy_density(weights) measurement")
    ap.add_argument("--single", metavar="PARENT_LIB", help="the single solve against the parent commit's library, in fresh processes")
    ap.add_argument("--single-child", metavar="NAME", choices=list(SIZES), help=argparse.SUPPRESS)
    ap.add_argument("--k1", metavar="LIB", help="the K1 A/B, with a library that holds both kernels and the probe")
    ap.add_argument("--k1-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--demo", action="store_true", help="the sensor-temperature descent")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if a.single_child:
        single_child(a.single_child, a.reps)
        return
    if a.k1_child:
        k1_child(a.launches, a.rounds)
        return
    os.makedirs(a.out, exist_ok=True)
    if a.single:
        single_ab(a.single, a.reps, a.rounds, a.out)
        return
    if a.k1:
        runs = child(["--k1-child", "--launches", str(a.launches), "--rounds", str(a.rounds)], a.k1)
        for r in runs:
            print(json.dumps(r), flush=True)
        json.dump({"cmd": "python tools/elliptic_many_bench.py --k1 LIB --launches %d --rounds %d" % (a.launches, a.rounds), "ms_per_launch": runs},
                  open(os.path.join(a.out, "k1_ab.json"), "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.demo:
        demo(lsm, a.steps)
        return
    path = os.path.join(a.out, "elliptic_many_bench.json")
    doc = {"cmd": "python tools/elliptic_many_bench.py --reps %d --cases %s --K %s" % (a.reps, " ".join(a.cases), " ".join(map(str, a.K))),
           "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL, "precond": "mg", "solves": [], "energy": []}
    for name in a.cases:        # the file is rewritten after every case: a long one may be cut short
        doc["solves"] += run(lsm, name, a.K, a.reps)
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)
    for name in a.energy:
        doc["energy"].append(run_energy(lsm, name, a.reps))
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
