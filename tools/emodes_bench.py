#!/usr/bin/env python
"""elliptic_modes on the device: writes profiles/emodes/emodes_bench.json (and prints one JSON line per case and block size), and the
evidence that moving the LOBPCG core into csrc/lobpcg.h changed nothing for elasticity_modes: profiles/emodes/refactor_bits.json.

The workload, fp64: tools/elliptic_bench.py's plate (block) with two circular (spherical) holes, ersatz contrast 1e-3, ρ_out = 1e-6,
u = 0 on the face x = 0; the m = 1, 4, 8 lowest modes at rtol 1e-6 from the default start, V-cycle preconditioner; at 512², 2048² and 128³.
  ms_per_solve      median, min, max of --reps solves of one EllipticModes object after a warm-up solve (the start vector, the first
                    Rayleigh–Ritz step, every iteration's two status reads and the host's small eigenproblems included), timed by the
                    host clock around a device synchronise, profiler off
  iterations        block iterations; vcycles: preconditioner applications (one per unconverged column and iteration)
  ms_per_iteration  ms_per_solve / iterations;  active = vcycles / iterations, the mean number of unconverged columns
  yardstick         ms per PCG iteration of elliptic_solve on the same operator, measured in the same process (f = 1, rtol 1e-8) × active:
                    one V-cycle and one apply per active column is what a block iteration cannot do without; `ratio` =
                    ms_per_iteration / yardstick, the cost of the residual, Gram and update passes and of the host's part on top
  block_apply       lsm_elliptic_modes_apply at ncols = 1, 4, 8 against ncols launches of lsm_elliptic_apply, interleaved, --apply-launches
                    launches per timed window: µs per call of each, their ratio, and the block apply's bytes model (8 + 16·ncols) B per
                    node (the cells once; x read and y written per column; the mask byte and the neighbours' x from the cache) as GB/s
                    and as a fraction of `--copy-tbs` (tools/copy_bw, 8 bytes per lane, read + write; run when the option is absent)
Kernel shares: run `--no-write --only NAME --m M` under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR`, a run of its own,
then `--stats DIR --only NAME --m M` adds every el_*, elm_*, em_* and mg_* kernel's dispatches, total time and share to the file.

--refactor PARENT_LIB: elasticity_modes from the parent commit's library and from this one (LSM_AMD_LIB selects it; a fresh process per
run, parent and new alternating, twice each): for two rows of tests/_modes_ref.cases() the SHA-256 of vectors() and the eigenvalues' bits
must be identical, and at 512², m = 4, the ms per solve of each run.  The bar for "no change" is the spread of parent against parent."""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from elliptic_bench import SIZES as ELLIPTIC_SIZES, copy_yardstick, field, summary, two_holes

OUT = os.path.join(ROOT, "profiles", "emodes")
SIZES = {k: ELLIPTIC_SIZES[k] for k in ("512x512", "2048x2048", "128c")}
BLOCKS = (1, 4, 8)
RTOL = 1e-6
BIT_ROWS = ("33x33_m4", "17c_m6")


def timed(b, fn, reps):
    ts = []
    for _ in range(reps):
        b.sync()
        t = time.perf_counter()
        fn()
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def block_apply(b, op, md, nn, launches, copy_tbs):
    t = b.torch
    lib, h = b.lib, md._handle()
    x = t.randn(8 * nn, dtype=t.float64, device=b.device)
    y = t.empty_like(x)
    xs, ys = [x[k * nn:(k + 1) * nn] for k in range(8)], [y[k * nn:(k + 1) * nn] for k in range(8)]
    out = []
    for ncols in BLOCKS:
        def blk():
            for _ in range(launches):
                lib.lsm_elliptic_modes_apply(h, ncols, b.ptr(x), b.ptr(y))

        def single():
            for _ in range(launches):
                for k in range(ncols):
                    lib.lsm_elliptic_apply(op._handle(), b.ptr(xs[k]), b.ptr(ys[k]))

        blk(), single()      # warm-up
        tb, ts = [], []
        for _ in range(5):   # interleaved
            tb += timed(b, blk, 1)
            ts += timed(b, single, 1)
        us_b, us_s = 1e3 * float(np.median(tb)) / launches, 1e3 * float(np.median(ts)) / launches
        r = {"ncols": ncols, "block_us": round(us_b, 2), "singles_us": round(us_s, 2), "singles_over_block": round(us_s / us_b, 3), "launches_per_window": launches,
             "model_bytes_per_node": 8 + 16 * ncols, "model_gbs": round((8 + 16 * ncols) * nn / (us_b * 1e-6) / 1e9, 1)}
        if copy_tbs:
            r["frac_of_copy"] = round(r["model_gbs"] / (copy_tbs * 1e3), 3)
        out.append(r)
    return out


def run(lsm, name, blocks, reps, launches, copy_tbs, apply_too=True):
    n = SIZES[name]
    nn = int(np.prod(n))
    eq, phi = field(lsm, n, two_holes(n))
    b = phi.backend
    op = lsm.EllipticOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    f = b.node_array(1.0, "f")
    sol = op.solve(f, rtol=1e-8, max_iters=200000)
    pcg = float(np.median(timed(b, lambda: op.solve(f, rtol=1e-8, max_iters=200000), reps))) / sol.iterations
    out = []
    for m in blocks:
        res = {"case": name, "n": list(n), "unknowns": nn, "m": m, "reps": reps, "levels": op.levels, "pcg_ms_per_iteration": round(pcg, 4), "pcg_iterations": sol.iterations}
        b.sync()
        t = time.perf_counter()
        md = op.modes(m, rtol=RTOL, max_iters=2000)         # the warm-up solve, the mass included
        b.sync()
        res["first_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        res.update(summary(timed(b, lambda: md.solve(rtol=RTOL, max_iters=2000), reps)))
        res.update(iterations=md.iterations, vcycles=md.stats[1], dropped=md.stats[2], relres=float(md.relres.max()), eigenvalues=[float(v) for v in md.eigenvalues])
        res["ms_per_iteration"] = round(res["ms_per_solve"] / max(md.iterations, 1), 4)
        res["active"] = round(md.stats[1] / max(md.iterations, 1), 3)
        res["yardstick_ms"] = round(pcg * res["active"], 4)
        res["ratio"] = round(res["ms_per_iteration"] / res["yardstick_ms"], 3)
        if apply_too and m == blocks[-1]:
            res["block_apply"] = block_apply(b, op, md, nn, launches, copy_tbs)
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
        k = re.search(r"\b(el|elm|em|mg)_\w+_kernel(<[\w:, ]+>)?", r["Name"].split("(")[0])
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


# ---- the refactor's evidence: one run of elasticity_modes per process, the library chosen by LSM_AMD_LIB

def elastic_child(reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _modes_ref as R
    import lsm_amd as lsm
    from elastic_bench import SIZES as ES, field as efield, two_holes as eholes
    # the parent's library has no lsm_elliptic_modes_*: this run calls none of them, so they are not looked up in it
    lsm._lib._SIGS[:] = [s for s in lsm._lib._SIGS if not s[0].startswith("lsm_elliptic_modes_")]
    res = {"lib": os.path.relpath(lsm._lib.LIB_PATH, ROOT), "rows": {}}
    for name in BIT_ROWS:
        cs = R.cases()[name]
        n = cs["n"]
        mf = lsm.MeshField(np.asfortranarray(cs["phi"]), lsm.CartesianGrid((0.0,) * len(n), cs["hc"], n), dtype=cs["dtype"])
        phi = lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()
        mask = np.stack([(cs["bits"] >> i) & 1 != 0 for i in range(len(n))], axis=-1)
        op = lsm.ElasticityOperator(phi, E_in=cs["E_in"], E_out=cs["E_out"], nu=cs["nu"], plane=cs["plane"], dirichlet=(mask, 0.0), precond=cs["precond"])
        md = op.modes(cs["m"], rho_in=cs["rho_in"], rho_out=cs["rho_out"], max_iters=600)
        res["rows"][name] = {"vectors_sha256": hashlib.sha256(np.ascontiguousarray(md.vectors()).tobytes()).hexdigest(),
                             "eigenvalue_bits": [float(v).hex() for v in md.eigenvalues], "iterations": md.iterations}
        md.close()
        op.close()
        phi.backend.close()
    n = ES["512x512"]
    eq, phi = efield(lsm, n, eholes(n))
    b = phi.backend
    op = lsm.ElasticityOperator(phi, dirichlet=(lsm.face_mask(phi.mesh, 0, 0), 0.0))
    md = op.modes(4, rtol=RTOL, max_iters=2000)
    res["512x512_m4"] = {**summary(timed(b, lambda: md.solve(rtol=RTOL, max_iters=2000), reps)), "iterations": md.iterations,
                         "vectors_sha256": hashlib.sha256(np.ascontiguousarray(md.vectors()).tobytes()).hexdigest()}
    md.close()
    op.close()
    eq.backend.close()
    print("CHILD " + json.dumps(res), flush=True)


def refactor(parent_lib, reps, out):
    new_lib = os.path.join(ROOT, "levelsetmethods.jl_amd", "libhiplsm.so")
    runs = []
    for which, lib in (("parent", parent_lib), ("new", new_lib), ("parent", parent_lib), ("new", new_lib)):
        env = dict(os.environ, LSM_AMD_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--elastic-child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=600)
        line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD ")), None)
        if p.returncode != 0 or line is None:
            sys.exit("the %s run failed (%d):\n%s\n%s" % (which, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
        r = json.loads(line[6:])
        r["which"] = which
        print(json.dumps(r), flush=True)
        runs.append(r)
    par, new = [r for r in runs if r["which"] == "parent"], [r for r in runs if r["which"] == "new"]
    same = all(r["rows"] == par[0]["rows"] and r["512x512_m4"]["vectors_sha256"] == par[0]["512x512_m4"]["vectors_sha256"] for r in runs)
    pm, nm = [r["512x512_m4"]["ms_per_solve"] for r in par], [r["512x512_m4"]["ms_per_solve"] for r in new]
    doc = {"cmd": "python tools/emodes_bench.py --refactor PARENT_LIB --reps %d" % reps, "device": "MI355X (gfx950), 1 GPU", "rows": list(BIT_ROWS),
           "bits_identical": same, "parent_ms_per_solve": pm, "new_ms_per_solve": nm, "parent_spread_ms": round(abs(pm[0] - pm[1]), 3),
           "new_minus_parent_ms": round(float(np.mean(nm) - np.mean(pm)), 3), "runs": runs}
    doc["new_spread_ms"] = round(abs(nm[0] - nm[1]), 3)
    doc["verdict"] = ("no change" if abs(doc["new_minus_parent_ms"]) <= doc["parent_spread_ms"] else
                      "slower than the parent's own spread: a finding to explain" if doc["new_minus_parent_ms"] > 0 else "not slower")
    json.dump(doc, open(os.path.join(out, "refactor_bits.json"), "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("bits_identical", "parent_ms_per_solve", "new_ms_per_solve", "parent_spread_ms", "new_spread_ms", "new_minus_parent_ms", "verdict")}))
    if not same:
        sys.exit("elasticity_modes differs between the parent's library and this one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--only", choices=list(SIZES), help="one case (the run under the profiler, or with --stats the case the trace is of)")
    ap.add_argument("--m", type=int, choices=BLOCKS, help="with --only: one block size")
    ap.add_argument("--apply-launches", type=int, default=50, help="block-apply launches per timed window")
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", metavar="DIR", help="add the kernel statistics of a --kernel-trace --stats directory to the existing file, run nothing")
    ap.add_argument("--refactor", metavar="PARENT_LIB", help="compare elasticity_modes between the parent commit's library and this one; run nothing else")
    ap.add_argument("--elastic-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/emodes)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    if a.elastic_child:
        return elastic_child(a.reps)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "emodes_bench.json")
    if a.refactor:
        return refactor(a.refactor, a.reps, a.out)
    if a.stats:
        doc = json.load(open(path))
        tr = doc.setdefault("kernel_trace", {"cmd": "rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/emodes_bench.py --no-write --only NAME "
                                                    "--m M; python tools/emodes_bench.py --stats <dir> --only NAME --m M",
                                             "note": "one traced run, the operator's setup, the PCG yardstick's solves and the warm-up solve included (traced, so slower "
                                                     "than the plain run)",
                                             "cases": {}})
        tr["cases"]["%s m=%s" % (a.only, a.m)] = kernel_stats(a.stats)
        json.dump(doc, open(path, "w"), indent=1)
        return
    copy_tbs = None if a.only else a.copy_tbs if a.copy_tbs else copy_yardstick()      # its own process, before this one touches the device
    import lsm_amd as lsm
    if a.only:
        run(lsm, a.only, (a.m,) if a.m else BLOCKS, a.reps, a.apply_launches, None, apply_too=False)
        return
    doc = {"cmd": "python tools/emodes_bench.py --reps %d --cases %s" % (a.reps, " ".join(a.cases)), "device": "MI355X (gfx950), 1 GPU", "rtol": RTOL,
           "contrast": 1e-3, "rho_out": 1e-6, "copy_tbs_8B_per_lane": copy_tbs,
           "yardstick": "elliptic_solve's mg ms per PCG iteration on the same operator, measured in the same process, × active columns", "cases": []}
    for name in a.cases:        # the file is rewritten after every case: the largest one may be cut short
        doc["cases"].extend(run(lsm, name, BLOCKS, a.reps, a.apply_launches, copy_tbs))
        if not a.no_write:
            json.dump(doc, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
