#!/usr/bin/env python
"""elasticity_modes on the device: writes profiles/modes/modes_bench.json (and prints one JSON line per case and block size).

The workload, fp64: tools/elastic_bench.py's plate (block) with two circular (spherical) holes, ersatz contrast 1e-3, ρ_out = 1e-6,
ν = 0.3, clamped on the face x = 0; the m = 1, 4, 8 lowest modes at rtol 1e-6 from the default start, V-cycle preconditioner; at 512²,
2048² and 128³.
  ms_per_solve      median, min, max of --reps solves of one ElasticityModes object after a warm-up solve (the start vector, the first
                    Rayleigh–Ritz step, every iteration's two status reads and the host's small eigenproblems included)
  iterations        block iterations; vcycles: preconditioner applications (one per unconverged column and iteration)
  ms_per_iteration  ms_per_solve / iterations;  active = vcycles / iterations, the mean number of unconverged columns
  yardstick         ms per PCG iteration of elasticity_solve on the same operator (profiles/elastic/elastic_bench.json, mg) × active:
                    one V-cycle and one apply per active column is what a block iteration cannot do without; `ratio` =
                    ms_per_iteration / yardstick, the cost of the residual, Gram and update passes and of the host's part on top
Kernel shares: run `--no-write --only NAME --m M` under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, a run of its own,
then `--stats DIR --only NAME --m M` adds every es_* and em_* kernel's dispatches, total time and share to the file."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from elastic_bench import SIZES as ELASTIC_SIZES, field, summary, two_holes

OUT = os.path.join(ROOT, "profiles", "modes")
SIZES = {k: ELASTIC_SIZES[k] for k in ("512x512", "2048x2048", "128c")}
BLOCKS = (1, 4, 8)
RTOL = 1e-6


def pcg_ms_per_iteration(name):
    try:
        doc = json.load(open(os.path.join(ROOT, "profiles", "elastic", "elastic_bench.json")))
        return next(c["mg"]["ms_per_iteration"] for c in doc["cases"] if c["case"] == name)
    except (OSError, StopIteration, KeyError):
        return None


def run(lsm, name, blocks, reps):
    n = SIZES[name]
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    pcg = pcg_ms_per_iteration(name)
    out = []
    for m in blocks:
        res = {"case": name, "n": list(n), "unknowns": len(n) * int(np.prod(n)), "m": m, "reps": reps, "levels": op.levels}
        b.sync()
        t = time.perf_counter()
        md = op.modes(m, rtol=RTOL, max_iters=2000)         # the warm-up solve, the mass included
        b.sync()
        res["first_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        ts = []
        for _ in range(reps):
            b.sync()
            t = time.perf_counter()
            md.solve(rtol=RTOL, max_iters=2000)
            b.sync()
            ts.append((time.perf_counter() - t) * 1e3)
        res.update(summary(ts))
        res.update(iterations=md.iterations, vcycles=md.stats[1], dropped=md.stats[2], relres=float(md.relres.max()), eigenvalues=[float(v) for v in md.eigenvalues])
        res["ms_per_iteration"] = round(res["ms_per_solve"] / max(md.iterations, 1), 4)
        res["active"] = round(md.stats[1] / max(md.iterations, 1), 3)
        if pcg:
            res["yardstick_ms"] = round(pcg * res["active"], 4)
            res["ratio"] = round(res["ms_per_iteration"] / res["yardstick_ms"], 3)
        print(json.dumps(res), flush=True)
        out.append(res)
        md.close()
    op.close()
    eq.backend.close()
    return out


def kernel_stats(dirname):
    f = glob.glob(dirname + "/**/*kernel_stats.csv", recursive=True)[0]
    out = {}
    for r in csv.DictReader(open(f)):
        k = re.search(r"\b(es|em|mg)_\w+_kernel(<[\w:, ]+>)?", r["Name"].split("(")[0])
        if not k:
            continue
        e = out.setdefault(k.group(0), {"dispatches": 0, "total_ms": 0.0})
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--only", choices=list(SIZES), help="one case (the run under the profiler, or with --stats the case the trace is of)")
    ap.add_argument("--m", type=int, choices=BLOCKS, help="with --only: one block size")
    ap.add_argument("--stats", metavar="DIR", help="add the kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/modes)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "modes_bench.json")
    if a.stats:
        doc = json.load(open(path))
        tr = doc.setdefault("kernel_trace", {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/modes_bench.py --no-write --only NAME "
                                                    "--m M; python tools/modes_bench.py --stats <dir> --only NAME --m M",
                                             "note": "one traced run, the operator's setup and the warm-up solve included (traced, so slower than the plain run)",
                                             "cases": {}})
        tr["cases"]["%s m=%s" % (a.only, a.m)] = kernel_stats(a.stats)
        json.dump(doc, open(path, "w"), indent=1)
        return
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, (a.m,) if a.m else BLOCKS, a.reps)
        return
    doc = {"cmd": "python tools/modes_bench.py --reps %d --cases %s" % (a.reps, " ".join(a.cases)), "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL,
           "contrast": 1e-3, "rho_out": 1e-6, "nu": 0.3, "yardstick": "profiles/elastic/elastic_bench.json: mg ms_per_iteration × active columns", "cases": []}
    for name in a.cases:        # the file is rewritten after every case: the largest one may be cut short
        doc["cases"].extend(run(lsm, name, BLOCKS, a.reps))
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
