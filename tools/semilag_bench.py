#!/usr/bin/env python
"""SemiLagrangian on the device: writes profiles/semilag/semilag_bench.json (and prints one JSON line per measurement).

Every measurement runs in a fresh process (a child of this script), the variants of a comparison interleaved (A B A B), after
200 ms of the same load (steady clocks); the figure of a variant is the median of its runs.

  steps     ms per lsm_advance_semilag (ghost fill + counters + the gather pass) at cfl 4 for orders 1 / 3 / 5, LSM_SEMILAG_STAGE = 1
            (staged tiles) against 0 (direct gather), with the workgroup counts of the staged launch, against the traffic model
            of one read and one write of ϕ (16 B per node in fp64) at the rate of `--copy-tbs` (tools/copy_bw, 8 bytes per lane,
            read + write; run when the option is absent and the program is built)
  to_tf     (two interleaved rounds, the runs of each variant recorded) wall time of integrate_ — with the counters it reads after every
            step, one small reduction and a host wait — to the same tf (10 SemiLagrangian steps at cfl 4 of the initial velocity): SemiLagrangian(4),
            RK3 + WENO5 and RK3 + Upwind (cfl 0.5) of this tree and, with --parent-lib, of the parent commit's library
            (LSM_AMD_LIB selects it; it has no lsm_advance_semilag, so the child takes that symbol out of the binding first)
  --nostats (a run of its own, semilag_nostats.json): integrate_ to that tf with and without the counters, SemiLagrangian(stats=False)
  vortex    tools/i2oe_bench.py's 256³ vortex case to its tf (10 I2OE steps at cfl 2): SemiLagrangian and SemiImplicitI2OE at
            cfl 2 and 4

Cases: the rotation of the off-centre disk at 2048², LeVeque's vortex deformation at 256³ and 512³, NeumannBC, fp64."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "semilag")
SIZES = {"2048x2048": (2048, 2048), "256x256x256": (256, 256, 256), "512x512x512": (512, 512, 512)}


def copy_yardstick():
    """TB/s (read + write) of tools/copy_bw's 8-bytes-per-lane copy, one element per thread"""
    exe = os.path.join(ROOT, "tools", "copy_bw")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"8 B/lane, one element per thread\s+[\d.]+ ms\s+([\d.]+) TB/s", out)
    return float(m.group(1)) if m else None


# ----------------------------------------------------------------------------- children: one measurement per process
def _case(lsm, np, n):
    if len(n) == 2:
        g = lsm.CartesianGrid((-1, -1), (1, 1), n)
        return g, lsm.MeshField(lambda x: np.hypot(x[0] - 0.4, x[1]) - 0.3, g), lsm.RigidRotation()
    g = lsm.CartesianGrid((0, 0, 0), (1, 1, 1), n)
    ic = lsm.MeshField(lambda x: np.sqrt((x[0] - 0.35) ** 2 + (x[1] - 0.35) ** 2 + (x[2] - 0.35) ** 2) - 0.15, g)
    return g, ic, lsm.vortex_deformation(g)


def child(a):
    if a.without_semilag:   # the parent commit's library: the binding must not ask it for the new symbol
        import lsm_amd
        lsm_amd._lib._SIGS[:] = [s for s in lsm_amd._lib._SIGS if s[0] != "lsm_advance_semilag"]
    import numpy as np
    import torch

    import lsm_amd as lsm
    n = tuple(int(x) for x in a.n.split(","))
    grid, ic, vel = _case(lsm, np, n)
    sync = torch.cuda.synchronize
    if a.child == "step":
        eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel, lsm.Upwind()), ic=ic, bc=lsm.NeumannBC(), integrator=lsm.SemiLagrangian(a.cfl, order=a.order),
                                  tuning={"LSM_SEMILAG_STAGE": a.stage})
        dt = a.cfl * eq.compute_cfl(0.0)
        terms = lsm.api._terms_c(eq.terms)
        p, q = eq.state.buf, eq.backend.alloc()
        stats = eq.backend.advance_semilag(terms, p, q, 0.0, dt, a.order, 2, True)
        step = lambda x, y: eq.backend.advance_semilag(terms, x, y, 0.0, dt, a.order, 2, True, want_stats=False)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:
            for _ in range(5):
                step(q, p)
                step(p, q)
            sync()
        t0 = time.perf_counter()
        for _ in range(a.steps // 2):
            step(q, p)
            step(p, q)
        sync()
        ms = (time.perf_counter() - t0) * 1e3 / (2 * (a.steps // 2))
        print("CHILD " + json.dumps({"ms_per_step": ms, "staged": stats[0], "fallback": stats[1], "max_cells": stats[2], "dt": dt, "device": torch.cuda.get_device_name(0)}), flush=True)
        return
    # time to tf
    integ, scheme = {"semilag": (lsm.SemiLagrangian(a.cfl, order=a.order), lsm.Upwind()),
                     "semilag_nostats": (lsm.SemiLagrangian(a.cfl, order=a.order, stats=False), lsm.Upwind()), "rk3weno5": (lsm.RK3(), lsm.WENO5()),
                     "rk3upwind": (lsm.RK3(), lsm.Upwind()), "i2oe": (lsm.SemiImplicitI2OE(cfl=a.cfl), lsm.Upwind())}[a.integ]
    probe = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel, lsm.Upwind()), ic=ic, bc=lsm.NeumannBC(), integrator=lsm.RK3())
    tf = a.tf_cfl_steps * probe.compute_cfl(0.0)
    probe.backend.close()
    times, steps = [], 0
    for _ in range(a.reps + 1):   # the first run warms up and is not counted
        eq = lsm.LevelSetEquation(terms=lsm.AdvectionTerm(vel, scheme), ic=ic, bc=lsm.NeumannBC(), integrator=integ)
        cnt = [0]
        sync()
        t0 = time.perf_counter()
        lsm.integrate_(eq, tf, posthook=lambda e: cnt.__setitem__(0, cnt[0] + 1))
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
        steps = cnt[0]
        eq.backend.close()
    print("CHILD " + json.dumps({"ms_to_tf": statistics.median(times[1:]), "steps": steps, "tf": tf, "device": torch.cuda.get_device_name(0)}), flush=True)


def run_child(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["LSM_AMD_LIB"] = os.path.abspath(lib)
        args = args + ["--without-semilag"]
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD ")), None)
    if p.returncode != 0 or line is None:
        raise RuntimeError(f"child {args} failed ({p.returncode}): {p.stderr[-600:]}")
    return json.loads(line[6:])


DEVICE = [None]   # what the runtime of the first child calls the device


def interleaved(variants, rounds):
    """variants: {name: (child args, library or None)}; A B … A B …; the runs of every variant"""
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (args, lib) in variants.items():
            runs[k].append(run_child(args, lib))
            DEVICE[0] = DEVICE[0] or runs[k][-1].get("device")
    return runs


def nostats(a):
    """what reading the counters after every step costs integrate_"""
    doc = {"cmd": "python tools/semilag_bench.py --nostats --cases " + " ".join(a.cases), "device": None, "rounds": a.tf_rounds, "cases": []}
    for name in a.cases:
        tf = ["--child", "tf", "--n", ",".join(map(str, SIZES[name])), "--reps", str(a.reps), "--tf-cfl-steps", "40", "--cfl", "4", "--integ"]
        r = interleaved({"stats": (tf + ["semilag"], None), "nostats": (tf + ["semilag_nostats"], None)}, a.tf_rounds)
        rec = {"case": name, "steps": r["stats"][0]["steps"]}
        for k, rs in r.items():
            rec[k + "_ms_to_tf"] = round(statistics.median(x["ms_to_tf"] for x in rs), 3)
            rec[k + "_runs_ms"] = [round(x["ms_to_tf"], 3) for x in rs]
        doc["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        doc["device"] = DEVICE[0]
        json.dump(doc, open(os.path.join(a.out, "semilag_nostats.json"), "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--orders", default="1,3,5")
    ap.add_argument("--rounds", type=int, default=2, help="runs of every variant of an interleaved comparison")
    ap.add_argument("--tf-rounds", type=int, default=2, help="runs of every variant of the time-to-tf comparison (each child times --reps runs)")
    ap.add_argument("--steps", type=int, default=40, help="timed steps per run")
    ap.add_argument("--reps", type=int, default=2, help="timed integrate_ runs per child")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--parent-lib", help="libhiplsm.so of the parent commit: its RK3 steps are timed next to the tree's")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/semilag)")
    ap.add_argument("--nostats", action="store_true",
                    help="only: integrate_ to the same tf with SemiLagrangian(4) and SemiLagrangian(4, stats=False), interleaved; writes semilag_nostats.json")
    ap.add_argument("--skip", default="", help="comma list of sections to skip: steps,to_tf,vortex")
    # children
    ap.add_argument("--child", choices=["step", "tf"], help=argparse.SUPPRESS)
    ap.add_argument("--n", help=argparse.SUPPRESS)
    ap.add_argument("--order", type=int, default=3, help=argparse.SUPPRESS)
    ap.add_argument("--stage", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--cfl", type=float, default=4.0, help=argparse.SUPPRESS)
    ap.add_argument("--integ", default="semilag", help=argparse.SUPPRESS)
    ap.add_argument("--tf-cfl-steps", type=float, default=40.0, help=argparse.SUPPRESS)
    ap.add_argument("--without-semilag", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    if a.nostats:
        return nostats(a)
    path = os.path.join(a.out, "semilag_bench.json")
    skip = set(a.skip.split(","))
    copy = a.copy_tbs or copy_yardstick()
    doc = {"cmd": "python tools/semilag_bench.py" + (" --parent-lib PARENT_LIB" if a.parent_lib else ""), "device": None, "dtype": "float64",
           "copy_tbs": copy, "model_bytes_per_node": 16, "rounds": a.rounds, "timed_steps": a.steps, "steps": [], "to_tf": [], "vortex": []}

    def save():
        doc["device"] = DEVICE[0]
        json.dump(doc, open(path, "w"), indent=1)
    med = lambda rs, key: statistics.median(r[key] for r in rs)
    for name in a.cases:
        n = SIZES[name]
        nn = 1
        for m in n:
            nn *= m
        ns = ",".join(map(str, n))
        model_ms = 16 * nn / (copy * 1e12) * 1e3 if copy else None
        if "steps" not in skip:
            for order in (int(o) for o in a.orders.split(",")):
                base = ["--child", "step", "--n", ns, "--order", str(order), "--steps", str(a.steps)]
                r = interleaved({"staged": (base + ["--stage", "1"], None), "direct": (base + ["--stage", "0"], None)}, a.rounds)
                rec = {"case": name, "order": order, "cfl": 4.0, "staged_ms": round(med(r["staged"], "ms_per_step"), 4),
                       "direct_ms": round(med(r["direct"], "ms_per_step"), 4), "staged_runs_ms": [round(x["ms_per_step"], 4) for x in r["staged"]],
                       "direct_runs_ms": [round(x["ms_per_step"], 4) for x in r["direct"]], "staged_workgroups": r["staged"][0]["staged"],
                       "fallback_workgroups": r["staged"][0]["fallback"], "max_cells": r["staged"][0]["max_cells"], "model_ms": model_ms and round(model_ms, 4)}
                rec["direct_over_staged"] = round(rec["direct_ms"] / rec["staged_ms"], 3)
                if model_ms:
                    rec["staged_over_model"] = round(rec["staged_ms"] / model_ms, 2)
                    rec["direct_over_model"] = round(rec["direct_ms"] / model_ms, 2)
                doc["steps"].append(rec)
                print(json.dumps(rec), flush=True)
                save()
        if "to_tf" not in skip:
            tf = ["--child", "tf", "--n", ns, "--reps", str(a.reps), "--tf-cfl-steps", "40"]
            variants = {"semilag_cfl4": (tf + ["--integ", "semilag", "--cfl", "4"], None), "rk3weno5_tree": (tf + ["--integ", "rk3weno5"], None),
                        "rk3upwind_tree": (tf + ["--integ", "rk3upwind"], None)}
            if a.parent_lib:
                variants["rk3weno5_parent"] = (tf + ["--integ", "rk3weno5"], a.parent_lib)
                variants["rk3upwind_parent"] = (tf + ["--integ", "rk3upwind"], a.parent_lib)
            r = interleaved(variants, a.tf_rounds)
            rec = {"case": name, "tf": r["semilag_cfl4"][0]["tf"]}
            for k, rs in r.items():
                rec[k] = {"ms_to_tf": round(med(rs, "ms_to_tf"), 3), "steps": rs[0]["steps"], "runs_ms": [round(x["ms_to_tf"], 3) for x in rs]}
            ref = rec.get("rk3upwind_parent", rec["rk3upwind_tree"])["ms_to_tf"]
            rec["rk3upwind_over_semilag"] = round(ref / rec["semilag_cfl4"]["ms_to_tf"], 2)
            rec["rk3weno5_over_semilag"] = round(rec.get("rk3weno5_parent", rec["rk3weno5_tree"])["ms_to_tf"] / rec["semilag_cfl4"]["ms_to_tf"], 2)
            doc["to_tf"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
    if "vortex" not in skip:
        tf = ["--child", "tf", "--n", "256,256,256", "--reps", str(a.reps), "--tf-cfl-steps", "20"]   # 10 I2OE steps at cfl 2
        for cfl in (2, 4):
            r = interleaved({"semilag": (tf + ["--integ", "semilag", "--cfl", str(cfl)], None), "i2oe": (tf + ["--integ", "i2oe", "--cfl", str(cfl)], None)}, a.tf_rounds)
            rec = {"case": "vortex256", "cfl": cfl, "tf": r["semilag"][0]["tf"], "semilag_ms": round(med(r["semilag"], "ms_to_tf"), 3), "semilag_steps": r["semilag"][0]["steps"],
                   "semilag_runs_ms": [round(x["ms_to_tf"], 3) for x in r["semilag"]], "i2oe_ms": round(med(r["i2oe"], "ms_to_tf"), 3),
                   "i2oe_steps": r["i2oe"][0]["steps"], "i2oe_runs_ms": [round(x["ms_to_tf"], 3) for x in r["i2oe"]]}
            rec["i2oe_over_semilag"] = round(rec["i2oe_ms"] / rec["semilag_ms"], 1)
            doc["vortex"].append(rec)
            print(json.dumps(rec), flush=True)
            save()
    save()
    print("wrote", path)


if __name__ == "__main__":
    main()
