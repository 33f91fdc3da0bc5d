"""`--refactor PARENT_LIB` of tools/homog_bench.py and tools/hcond_bench.py: the evidence that moving the periodic cell-problem core into
csrc/cell_problem.h changed neither a bit nor the speed.  Writes profiles/cell_problem/refactor_bits.json and ab.json (each tool
adds its own cases to both).

The parent commit's library, built apart, against this tree's: LSM_AMD_LIB selects one, a fresh child process each, taken in turn,
ROUNDS times each in one session.  Per child and case (the tool's smallest 2-D and 3-D sizes with mg, the 2-D one with jacobi):
  bits    SHA-256 of correctors(), of the tensor's bytes and of sensitivity(W).values(), and the iteration list: identical in all runs
  speed   ms per solve (median of --reps after a warm-up), per tensor call and per sensitivity call (median of 5); per metric the
          tree's median over the rounds is at most the parent's median + 2·(the parent's max − min over its rounds)
          (profiles/mg_shared/ab.json's rule).  A case that fails is reported as failing."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "cell_problem")
CASES = (("256x256", "mg"), ("64c", "mg"), ("256x256", "jacobi"))
ROUNDS = 3
RTOL = 1e-8
METRICS = ("ms_per_solve", "ms_per_tensor", "ms_per_sensitivity")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(tool, make, tensor, reps):
    """one process, one library: `tool` is the bench module (SIZES, inclusion, field, timed), make(lsm, phi, precond) the object,
    tensor(hom) a fresh tensor from the device (not the object's cached one)"""
    import lsm_amd as lsm
    res = {"lib": os.path.relpath(lsm._lib.LIB_PATH, ROOT), "cases": {}}
    for name, precond in CASES:
        n = tool.SIZES[name]
        eq, phi = tool.field(lsm, n, tool.inclusion(n, 0.09 if len(n) == 2 else 0.1))
        b = phi.backend
        hom = make(lsm, phi, precond)
        hom.solve(rtol=RTOL, max_iters=50000)      # warm-up, and the first chunk's length
        s = tool.timed(b, lambda: hom.solve(rtol=RTOL, max_iters=50000), reps)
        K = len(hom.iterations)
        W = np.array([[1.0 + 0.25 * (p + q) + (p == q) for q in range(K)] for p in range(K)])
        res["cases"]["%s %s" % (name, precond)] = {
            "iterations": hom.iterations, "correctors_sha256": _sha(hom.correctors()), "tensor_sha256": _sha(tensor(hom)),
            "sensitivity_sha256": _sha(hom.sensitivity(W).values()), "ms_per_solve": s["ms"],
            "ms_per_tensor": tool.timed(b, lambda: tensor(hom), 5)["ms"], "ms_per_sensitivity": tool.timed(b, lambda: hom.sensitivity(W), 5)["ms"]}
        hom.close()
        eq.backend.close()
    print("CHILD " + json.dumps(res), flush=True)


def _merge(path, head, cases):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.update(head)
    doc.setdefault("cases", {}).update(cases)
    return doc


def refactor(tool_file, key, parent_lib, reps, out=None):
    out = out or OUT
    new_lib = os.path.join(ROOT, "levelsetmethods.jl_amd", "libhiplsm.so")
    runs = []
    for which, lib in (("parent", parent_lib), ("new", new_lib)) * ROUNDS:
        env = dict(os.environ, LSM_AMD_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(tool_file), "--refactor-child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=900)
        line = next((l for l in p.stdout.splitlines() if l.startswith("CHILD ")), None)
        if p.returncode != 0 or line is None:
            sys.exit("the %s run failed (%d):\n%s\n%s" % (which, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
        r = dict(json.loads(line[6:]), which=which)
        print(json.dumps(r), flush=True)
        runs.append(r)
    bits, ab = {}, {}
    for name in runs[0]["cases"]:
        rows = [{k: v for k, v in r["cases"][name].items() if not k.startswith("ms_")} for r in runs]
        bits["%s %s" % (key, name)] = {"identical": all(x == rows[0] for x in rows), "runs": [dict(which=r["which"], lib=r["lib"], **x) for r, x in zip(runs, rows)]}
        case = {"iterations_identical": all(x["iterations"] == rows[0]["iterations"] for x in rows)}
        for m in METRICS:
            par = [r["cases"][name][m] for r in runs if r["which"] == "parent"]
            new = [r["cases"][name][m] for r in runs if r["which"] == "new"]
            bound = round(statistics.median(par) + 2 * (max(par) - min(par)), 3)
            case[m] = {"parent": par, "head": new, "parent_median": statistics.median(par), "head_median": statistics.median(new),
                       "parent_spread": round(max(par) - min(par), 3), "bound": bound, "pass": statistics.median(new) <= bound}
        case["pass"] = case["iterations_identical"] and all(case[m]["pass"] for m in METRICS)
        ab["%s %s" % (key, name)] = case
    os.makedirs(out, exist_ok=True)
    cmd = "python tools/homog_bench.py --refactor PARENT_LIB --reps %d; python tools/hcond_bench.py --refactor PARENT_LIB --reps %d" % (reps, reps)
    bdoc = _merge(os.path.join(out, "refactor_bits.json"), {"cmd": cmd, "device": "MI355X (gfx950), 1 GPU",
                  "what": "the parent commit's library (built apart, loaded with LSM_AMD_LIB) and the library with csrc/cell_problem.h, a fresh process each, "
                          "taken in turn, %d times each: SHA-256 of correctors(), of the tensor's bytes, of sensitivity(W).values(), and the iterations" % ROUNDS}, bits)
    bdoc["bits_identical"] = all(c["identical"] for c in bdoc["cases"].values())
    adoc = _merge(os.path.join(out, "ab.json"), {"cmd": cmd,
                  "what": "the same runs: rounds 1-%d in one session on one MI355X; ms_per_solve is each run's median over %d solves of all correctors after a "
                          "warm-up, ms_per_tensor and ms_per_sensitivity each run's median over 5 calls" % (ROUNDS, reps),
                  "criterion": "iterations identical, and per metric head median <= parent median + 2*(parent max - min over its rounds)"}, ab)
    adoc["verdict"] = "pass" if all(c["pass"] for c in adoc["cases"].values()) else "fail: " + ", ".join(k for k, c in adoc["cases"].items() if not c["pass"])
    for name, doc in (("refactor_bits.json", bdoc), ("ab.json", adoc)):
        with open(os.path.join(out, name), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({"bits_identical": {k: bits[k]["identical"] for k in bits}, "pass": {k: ab[k]["pass"] for k in ab}}))
    if not all(b["identical"] for b in bits.values()):
        sys.exit("%s differs between the parent's library and this one" % key)
