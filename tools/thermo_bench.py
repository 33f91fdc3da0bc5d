#!/usr/bin/env python
"""Thermoelastic coupling on the device: writes profiles/thermoelastic/thermo_bench.json (and prints one JSON line per case).
DESIGN.md §7.29.

The workload, fp64, at 2048² and 256³: elastic_bench's block with two holes (ersatz contrast 1e-3 for the modulus and the conductivity),
clamped and held at T = 0 on x = 0, a uniform heat source, alpha = 1e-2, T_ref = 0.
  passes        ms per call (median, min, max of --reps after a warm-up, the stream synchronised around each) of the five passes on
                smooth fields given through with_displacement — load, source, stress (the M node fields), von_mises, sensitivity
                (with `minus`) — and of lsm_elastic_energy_mutual, which has the sensitivity pass's u and v traffic.
  model_gbs     MODEL bytes / ms against `--copy-tbs` (tools/copy_bw's 8-bytes-per-lane copy of the same run, read + write, when the
                option is absent and the program is built).  The model counts every array once, 8 bytes an entry: the load reads T and
                the cell moduli and writes N node arrays; the source reads v and the moduli and writes one; the stress pair reads u, T
                and the moduli, writes and reads the M (or one) cell arrays and writes as many node fields; the sensitivity reads u, v,
                T, minus and the moduli and writes one field; the mutual energy reads u, v and the moduli and writes one.
  whole         ThermoelasticSolution.sensitivity(l) (l: a unit axial traction on x = 1) next to its two adjoint solves run alone — the
                elastic adjoint A v = b_l and the heat adjoint of the source pass's q — at rtol 1e-8 with mg; `rest` is what the
                source pass, the heat mutual energy, the fused sensitivity pass, the objective's reduction and the host add.
  --ab LIB      lsm_elastic_energy_mutual of this tree against the library LIB of the parent commit (through LSM_AMD_LIB), alternating in
                fresh processes, --rounds times each; a process whose library has the thermal entry points times the sensitivity pass
                beside it (so LIB may also be a variant of this tree's kernels).  Writes mutual_ab.json, or --ab-file."""
import argparse
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

from elastic_bench import copy_yardstick, field, two_holes
from topo_bench import smooth_u

OUT = os.path.join(ROOT, "profiles", "thermoelastic")
SIZES = {"2048x2048": (2048, 2048), "256c": (256, 256, 256)}
KEYS = ("load", "source", "stress", "von_mises", "sensitivity", "energy_mutual")
NEW = ("lsm_elastic_thermal_load", "lsm_elastic_thermal_stress_cells", "lsm_elastic_thermal_stress", "lsm_elastic_thermal_source",
       "lsm_elastic_thermal_sensitivity")
ALPHA, T_REF, RTOL = 1e-2, 0.0, 1e-8


def model_bytes(N, n):
    nodes, cells = float(np.prod(n)), float(np.prod([m - 1 for m in n]))
    M = N * (N + 1) // 2
    return {"load": 8.0 * ((1 + N) * nodes + cells), "source": 8.0 * ((N + 1) * nodes + cells),
            "stress": 8.0 * ((N + 1 + M) * nodes + (1 + 2 * M) * cells), "von_mises": 8.0 * ((N + 2) * nodes + 3 * cells),
            "sensitivity": 8.0 * ((2 * N + 3) * nodes + cells), "energy_mutual": 8.0 * ((2 * N + 1) * nodes + cells)}


def timed(b, reps, call):
    spent = 0.0
    while spent < 50.0:      # the warm-up keeps the device busy for 50 ms at least
        b.sync()
        t = time.perf_counter()
        call()
        b.sync()
        spent += (time.perf_counter() - t) * 1e3
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        call()
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"ms_per_call": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def smooth_t(n):
    x = np.meshgrid(*[np.linspace(0.0, 1.0, m) for m in n], indexing="ij", sparse=True)
    return np.asfortranarray(sum(np.cos(2.0 * xi + 0.3 * i) for i, xi in enumerate(x)) + np.zeros(n))


def setup(lsm, n):
    eq, phi = field(lsm, n, two_holes(n))
    clamp = lsm.face_mask(phi.mesh, 0, 0)
    eop = lsm.ElasticityOperator(phi, dirichlet=(clamp, 0.0))
    return eq, phi, eop, clamp


def pass_calls(lsm, eop, n, thermal=True):
    """name → call, on smooth u, v, T and minus"""
    b, hd = eop.backend, eop._handle()
    N = len(n)
    su, sv = eop.with_displacement(smooth_u(n)), eop.with_displacement(smooth_u(n)[::-1])
    ub, vb = [c.buf for c in su.u], [c.buf for c in sv.u]
    new = lambda: lsm.ROCMeshField(b, eop.mesh, eop.bcs)
    g = new()
    calls = {"energy_mutual": lambda: b.elastic_energy_mutual(hd, ub, vb, g.buf)}
    if thermal:
        T, minus = new(), new()
        T.copy_(smooth_t(n))
        minus.copy_(smooth_t(n))
        outs = [new() for _ in range(N * (N + 1) // 2)]
        S = lsm._lib
        calls.update({
            "load": lambda: b.elastic_thermal_load(hd, T.buf, T_REF, ALPHA),
            "source": lambda: b.elastic_thermal_source(hd, vb, ALPHA),
            "stress": lambda: b.elastic_thermal_stress(hd, ub, T.buf, T_REF, ALPHA, S.STRESS_STRESS, [c.buf for c in outs]),
            "von_mises": lambda: b.elastic_thermal_stress(hd, ub, T.buf, T_REF, ALPHA, S.STRESS_VON_MISES, [outs[0].buf]),
            "sensitivity": lambda: b.elastic_thermal_sensitivity(hd, ub, vb, T.buf, T_REF, ALPHA, minus.buf, g.buf)})
    return calls, (su, sv, g)


def tip_load(b, n):
    """l: the unit traction along x on the face x = 1 as one flat device array, component-major"""
    t = b.torch
    f = t.zeros(len(n) * int(np.prod(n)), dtype=t.float64, device=b.device)
    f[t.arange(n[0] - 1, int(np.prod(n)), n[0], device=b.device)] = 2.0 * (n[0] - 1)
    return f


def run(lsm, name, reps, whole_reps):
    n = SIZES[name]
    N = len(n)
    eq, phi, eop, clamp = setup(lsm, n)
    b = phi.backend
    res = {"case": name, "n": list(n), "nodes": int(np.prod(n)), "reps": reps}
    calls, keep = pass_calls(lsm, eop, n)
    mb = model_bytes(N, n)
    for key in KEYS:
        r = timed(b, reps, calls[key])
        r["model_bytes"] = mb[key]
        r["model_gbs"] = round(mb[key] / (r["ms_per_call"] * 1e-3) / 1e9, 1)
        res[key] = r
    res["sensitivity_over_energy_mutual"] = round(res["sensitivity"]["ms_per_call"] / res["energy_mutual"]["ms_per_call"], 3)
    del calls, keep
    # the whole sensitivity() next to its two adjoint solves
    hop = lsm.EllipticOperator(phi, dirichlet=(clamp, 0.0))
    co = lsm.Thermoelastic(hop, eop, alpha=ALPHA, T_ref=T_REF)
    kw = dict(rtol=RTOL, max_iters=200000)
    l = tip_load(b, n)
    sol = co.solve(1.0, None, **kw)
    sens = sol.sensitivity(l, **kw)      # the warm-up, and the source of the heat adjoint
    src = sens.heat_adjoint._f
    tw, te, th = [], [], []
    for _ in range(whole_reps):
        for ts, call in ((tw, lambda: sol.sensitivity(l, **kw)),
                         (te, lambda: b.elastic_solve(eop._handle(), l, [c.buf for c in eop._fields(None, fixed="zero")], RTOL, 200000)),
                         (th, lambda: b.elliptic_solve(hop._handle(), src, hop._field(None, homogeneous=True).buf, RTOL, 200000))):
            b.sync()
            t = time.perf_counter()
            call()
            b.sync()
            ts.append((time.perf_counter() - t) * 1e3)
    med = lambda ts: round(statistics.median(ts), 3)
    res["whole"] = {"reps": whole_reps, "sensitivity_ms": med(tw), "elastic_adjoint_ms": med(te), "heat_adjoint_ms": med(th),
                    "rest_ms": round(med(tw) - med(te) - med(th), 3), "state_iterations": [sol.temperature.iterations, sol.displacement.iterations],
                    "adjoint_iterations": [sens.iterations, sens.heat_iterations], "value": sens.value}
    print(json.dumps(res), flush=True)
    del sol, sens
    co.close()
    eq.backend.close()
    return res


def ab_child(name, reps):
    import lsm_amd as lsm
    other = os.environ.get("LSM_AMD_LIB")
    thermal = True
    try:
        lsm._lib.lib()
    except AttributeError:      # the parent's library has no thermal entry points: load it without them
        lsm._lib._SIGS[:] = [s for s in lsm._lib._SIGS if s[0] not in NEW]
        thermal = False
    n = SIZES[name]
    eq, phi, eop, _ = setup(lsm, n)
    calls, keep = pass_calls(lsm, eop, n, thermal=thermal)
    r = {"case": name, "lib": os.path.basename(other) if other else "tree", "energy_mutual": timed(phi.backend, reps, calls["energy_mutual"])}
    if thermal:
        r["sensitivity"] = timed(phi.backend, reps, calls["sensitivity"])
    print(json.dumps(r), flush=True)
    eop.close()


def child(args, lib=None):
    """a fresh process of this tool, with LSM_AMD_LIB = lib or without it; its JSON lines"""
    env = dict(os.environ)
    env.pop("LSM_AMD_LIB", None)
    if lib:
        env["LSM_AMD_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (args, r.returncode, r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def ab(parent_lib, reps, rounds, cases, out, fname):
    doc = {"cmd": "python tools/thermo_bench.py --ab %s --reps %d --rounds %d" % (os.path.basename(parent_lib), reps, rounds), "device": "MI355X (gfx950), 1 GPU",
           "runs": []}
    for name in cases:
        for _ in range(rounds):
            for lib in (parent_lib, None):
                r = child(["--ab-child", name, "--reps", str(reps)], lib)[0]
                print(json.dumps(r), flush=True)
                doc["runs"].append(r)
    json.dump(doc, open(os.path.join(out, fname), "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--ab", metavar="PARENT_LIB", help="lsm_elastic_energy_mutual against the parent commit's library, in fresh processes")
    ap.add_argument("--ab-file", default="mutual_ab.json", help="the file --ab writes (another library than the parent's: another name)")
    ap.add_argument("--ab-child", metavar="NAME", choices=list(SIZES), help=argparse.SUPPRESS)
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/thermoelastic)")
    ap.add_argument("--no-write", action="store_true", help="print only")
    a = ap.parse_args()
    if a.ab_child:
        ab_child(a.ab_child, a.reps)
        return
    os.makedirs(a.out, exist_ok=True)
    if a.ab:
        ab(a.ab, a.reps, a.rounds, a.cases, a.out, a.ab_file)
        return
    import lsm_amd as lsm
    cases = [run(lsm, name, a.reps, a.whole_reps) for name in a.cases]
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        for r in cases:
            for key in KEYS:
                r[key]["frac_of_copy"] = round(r[key]["model_gbs"] / (copy_tbs * 1e3), 3)
    doc = {"cmd": "python tools/thermo_bench.py --reps %d --whole-reps %d" % (a.reps, a.whole_reps), "device": "MI355X (gfx950), 1 GPU",
           "copy_tbs_8B_per_lane": copy_tbs, "alpha": ALPHA, "t_ref": T_REF, "rtol": RTOL, "cases": cases}
    json.dump(doc, open(os.path.join(a.out, "thermo_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
