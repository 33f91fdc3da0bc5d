#!/usr/bin/env python3
"""Tabulate the compiler's kernel resource report and compare two of them.

    for f in lsm_elastic lsm_elliptic lsm_homog lsm_hcond; do
        hipcc -std=c++17 -O3 --offload-arch=gfx950 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage \
              -c levelsetmethods.jl_amd/csrc/$f.hip -o /dev/null 2> head/$f.log
    done                                   (and the same at the parent commit into parent/)
    tools/resource_usage.py head [parent]

Prints one line per kernel: SGPRs, VGPRs, AGPRs, scratch bytes per lane, waves per SIMD, SGPR and VGPR spills, LDS bytes.
With a second directory every kernel of it is looked up in the first by translation unit and demangled name (template
arguments that the first appends, 0 or EsU, are ignored: parameters defaulted since), and every figure must agree.
"""
import glob
import os
import re
import subprocess
import sys

KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
HEAD = ["SGPR", "VGPR", "AGPR", "scratch", "waves", "sspill", "vspill", "LDS"]


def parse(path):
    out, cur, src = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"(?:\./)?([\w.]+):\d+:\d+: remark: (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        f, body = m.group(1), m.group(2).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            src = f
            out.setdefault((cur), {"file": f})
            continue
        if cur is None:
            continue
        k, _, v = body.rpartition(":")
        if k.strip() in KEYS:
            out[cur][k.strip()] = v.strip()
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def table(logs):
    rows = {}
    for log in logs:
        tu = os.path.basename(log).rsplit(".", 1)[0]
        d = parse(log)
        dm = demangle(list(d))
        for k, v in d.items():
            name = re.sub(r"^void ", "", dm[k]).split("(")[0].replace("lsm::", "")
            rows[(tu, name)] = [v.get(x, "?") for x in KEYS]
    return rows


def main():
    args = sys.argv[1:]
    head = table(sorted(glob.glob(os.path.join(args[0], "*.log"))))
    print("%-14s %-86s " % ("file", "kernel") + " ".join("%7s" % h for h in HEAD))
    for (f, n), v in sorted(head.items()):
        print("%-14s %-86s " % (f, n) + " ".join("%7s" % x for x in v))
    if len(args) < 2:
        return 0
    parent = table(sorted(glob.glob(os.path.join(args[1], "*.log"))))
    bad = 0
    print("\nagainst the parent (%d kernels):" % len(parent))
    for (f, n), v in sorted(parent.items()):
        cands = [hn for (hf, hn) in head if hf == f and (hn == n or (n.endswith(">") and hn.startswith(n[:-1] + ", ") and re.fullmatch(r"(, (0|EsU))*>", hn[len(n) - 1:]))
                                                          or (not n.endswith(">") and hn == n + "<0>"))]
        if len(cands) != 1:
            print("  NO MATCH  %s %s -> %s" % (f, n, cands))
            bad += 1
            continue
        hv = head[(f, cands[0])]
        if hv != v:
            print("  DIFFERS   %s %s: parent %s, now %s" % (f, n, v, hv))
            bad += 1
    print("  %d of %d kernels differ from the parent" % (bad, len(parent)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
