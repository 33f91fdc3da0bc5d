#!/usr/bin/env python
"""render on the device: writes profiles/render/render_bench.json (and prints one JSON line per case and image size).

  brick_ms       lsm_render_refresh (the brick pass and the ring pass), stream synchronised before and after; against the field read
                 once (8 or 4 bytes per node, plus a byte per node of a band's mask) as GB/s and as a fraction of `--copy-tbs`, what
                 tools/copy_bw reaches on the same box with 8 bytes per lane, one element per thread (read + write; the tool is run
                 when the option is absent and the program is built)
  ms_per_draw    lsm_render_draw into device buffers, synchronised before and after, median of --reps after a warm-up of at least
                 --warm-ms of draws (the device leaves its idle power state); LSM_RENDER_SKIP = 1 and 0 interleaved draw by draw
  rays_per_s, samples_per_s   pixels and lattice samples t_k = t_in + k·dt up to each ray's hit (or to t_out) per second; the
                 samples are counted on the host from the depth image, the same number with and without skipping
Cases: the exact-distance sphere ‖x‖ − 0.5 in [−1, 1]³ at 256³ and 512³, and the narrow band (nlayers 3, float32 storage) of the
sphere at 768³ as in BASELINE config 5; images of 512 × 512 and 1920 × 1080 from Camera.fit's view along (1, 1, 1).
--stats DIR NAME writes the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of `--cases NAME` next to it."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

OUT = os.path.join(ROOT, "profiles", "render")
CASES = {"sphere256": (256, False), "sphere512": (512, False), "band768": (768, True)}
SIZES = {"512x512": (512, 512), "1920x1080": (1920, 1080)}
STYLE = [70, 130, 180, 255, 255, 255, 0.25, 0.5, 6]


def field(lsm, n, band):
    grid = lsm.CartesianGrid((-1.0,) * 3, (1.0,) * 3, (n,) * 3)
    ax = np.linspace(-1.0, 1.0, n)
    vals = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5
    if band:
        mf = lsm.NarrowBandMeshField(lsm.MeshField(np.asfortranarray(vals.astype(np.float32)), grid, dtype=np.float32), nlayers=3)
    else:
        mf = lsm.MeshField(np.asfortranarray(vals), grid)
    del vals
    return lsm.LevelSetEquation(terms=(lsm.NormalMotionTerm(0.0),), ic=mf, bc=lsm.NeumannBC()).current_state()


def lattice_samples(cam, W, H, depth, dt):
    """lattice samples up to each ray's hit, or to t_out: the slab test of the rules against [−1, 1]³ (perspective rays)"""
    eye, f, rs, us = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    sx = (2.0 * (np.arange(W) + 0.5)) / W - 1.0
    sy = 1.0 - (2.0 * (np.arange(H) + 0.5)) / H
    d = f[None, None, :] + sx[None, :, None] * rs[None, None, :] + sy[:, None, None] * us[None, None, :]
    d /= np.sqrt((d * d).sum(axis=2))[..., None]
    with np.errstate(all="ignore"):
        t1, t2 = (-1.0 - eye) / d, (1.0 - eye) / d
    tin = np.maximum(np.minimum(t1, t2).max(axis=2), 0.0)
    tout = np.maximum(t1, t2).min(axis=2)
    inside = tout > tin
    end = np.where(np.isfinite(depth), depth, tout)
    return int((np.floor((end - tin)[inside] / dt) + 1 + np.isfinite(depth)[inside]).sum())


def run(lsm, name, reps, warm_ms):
    n, band = CASES[name]
    phi = field(lsm, n, band)
    b = phi.backend
    r = b.render_create(phi.buf, phi.mask if band else None, 0.0)
    b.sync()
    ts = []
    for _ in range(reps + 1):
        b.sync()
        t = time.perf_counter()
        b.render_refresh(r)
        b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    brick_ms = statistics.median(ts[1:])
    tab = b.render_bricks(r)
    nbytes = n ** 3 * ((4 + 1) if band else 8)
    res = {"case": name, "n": n, "band": band, "storage": "float32" if band else "float64", "reps": reps, "brick_ms": round(brick_ms, 3),
           "bricks": int(tab.size), "uniform_bricks": int(((tab & 4) != 0).sum()), "brick_model_bytes": nbytes,
           "brick_model_gbs": round(nbytes / (brick_ms * 1e-3) / 1e9, 1), "images": []}
    cam_obj = lsm.Camera.fit(phi.mesh)
    dt = STYLE[7] * 2.0 / (n - 1)
    for sname, (W, H) in SIZES.items():
        cam = cam_obj.vectors(W, H)
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < warm_ms:
            b.render_draw(r, cam, W, H, STYLE)
            b.sync()
        ms = {1: [], 0: []}
        depth = None
        for _ in range(reps):
            for skip in (1, 0):
                b.set_tuning("LSM_RENDER_SKIP", skip)
                b.sync()
                t = time.perf_counter()
                out = b.render_draw(r, cam, W, H, STYLE)
                b.sync()
                ms[skip].append((time.perf_counter() - t) * 1e3)
                d = out[1].cpu().numpy()
                assert depth is None or np.array_equal(d, depth), "the picture differs between draws"
                depth = d
        b.set_tuning("LSM_RENDER_SKIP", 1)
        ns = lattice_samples(cam, W, H, depth, dt)
        e = {"size": sname, "rays": W * H, "hits": int(np.isfinite(depth).sum()), "lattice_samples": ns}
        for skip in (1, 0):
            m = statistics.median(ms[skip])
            e[f"skip{skip}"] = {"ms_per_draw": round(m, 3), "ms_min": round(min(ms[skip]), 3), "ms_max": round(max(ms[skip]), 3),
                                "rays_per_s": round(W * H / (m * 1e-3)), "samples_per_s": round(ns / (m * 1e-3))}
        e["skip_speedup"] = round(statistics.median(ms[0]) / statistics.median(ms[1]), 2)
        res["images"].append(e)
    b.render_destroy(r)
    print(json.dumps(res), flush=True)
    return res


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
        kname = r["Name"].split("(")[0].replace("void ", "")
        if "render_" not in kname:
            continue
        e = out.setdefault(kname, {"dispatches": 0, "total_ms": 0.0})
        e["dispatches"] += int(r["Calls"])
        e["total_ms"] += int(r["TotalDurationNs"]) / 1e6
    for e in out.values():
        e["total_ms"] = round(e["total_ms"], 3)
        e["us_per_dispatch"] = round(1e3 * e["total_ms"] / e["dispatches"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--copy-tbs", type=float, help="the copy yardstick in TB/s (default: run tools/copy_bw)")
    ap.add_argument("--stats", nargs=2, metavar=("DIR", "NAME"), help="write NAME_kernel_trace.json from a --kernel-trace --stats directory")
    ap.add_argument("--out", default=OUT, help="output directory (default: profiles/render)")
    ap.add_argument("--no-write", action="store_true", help="print only (the run under the profiler)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.stats:
        d, name = a.stats
        json.dump({"cmd": f"rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/render_bench.py --cases {name} --reps {a.reps} --no-write; "
                          f"python tools/render_bench.py --stats <dir> {name}",
                   "case": f"{name}: {a.reps + 2} brick passes, then per image size a warm-up and {a.reps} draws each with LSM_RENDER_SKIP = 1 "
                           "(render_ray_kernel<…, true>) and 0 (<…, false>)",
                   "nnode": CASES[name][0] ** 3, "kernels": kernel_stats(d)},
                  open(os.path.join(a.out, f"{name}_kernel_trace.json"), "w"), indent=1)
        return
    import lsm_amd as lsm
    res = [run(lsm, name, a.reps, a.warm_ms) for name in a.cases.split(",")]
    if a.no_write:
        return
    copy_tbs = a.copy_tbs if a.copy_tbs else copy_yardstick()
    if copy_tbs:
        for c in res:
            c["brick_frac_of_copy"] = round(c["brick_model_gbs"] / (copy_tbs * 1e3), 3)
    json.dump({"cmd": "python tools/render_bench.py --reps %d" % a.reps, "device": "MI355X (gfx950), 1 GPU", "copy_tbs_8B_per_lane": copy_tbs,
               "style": dict(zip(("color", "background", "ambient", "step", "bisections"), (STYLE[0:3], STYLE[3:6], *STYLE[6:]))), "cases": res},
              open(os.path.join(a.out, "render_bench.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
