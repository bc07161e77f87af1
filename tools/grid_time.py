#!/usr/bin/env python
"""What the closest-point grid scene (api.Scene_grid) costs and finds against the two associations it sits between, on the configs[1] / [2]
inputs: 256 obj_06 hypotheses, 640x480, 20 iterations, synchronous refine_batch (host clocks around the calls, after warm-up, the cases
INTERLEAVED call by call in one process; median / min / max ms):
  (a) projective scene   (b) kd-tree scene   (c) grid scene at each --cells size (default 1, 2 and 4 mm), built from (b).
Steps, each a child process of its own under its own time limit (the first one that fails ends the run):
  time-device / time-host   the table above in either solve mode, and poses/s;
  build                     the build (pr_scene_grid_build_dev) per cell size for the bench's scene and for a frame-filling one (the object in
                            front of a wall, 307 k points), the grids' sizes, next to the kd-tree scene's own device preparation;
  kernel                    one timed batch per scene (option profile = 1): the correspondence launches' time per launch;
  accuracy                  pr_pose_distance against synth.scene_pose(): ADD < 0.1 d, MSSD < 1 mm, median ADD for (a), (b), (c), and the largest
                            MSSD between the grid's and the kd-tree's refined pose of the same hypothesis.
One JSON line per step, then one with all of them.

    python tools/grid_time.py [--calls 20] [--warmup 3] [--cells 1,2,4] [--step NAME] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pose_refine_amd import api, synth  # noqa: E402

STEPS = ("time-device", "time-host", "build", "kernel", "accuracy")
W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
CRIT = (0.0, 0.0, 20)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def interleaved(cases, calls, warmup):
    """Every case once per round, round after round: drift of the box hits all cases alike."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    ms = {k: [] for k in cases}
    for _ in range(calls):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def timed(fn):
    api.sync(); t = time.perf_counter(); r = fn(); api.sync()
    return (time.perf_counter() - t) * 1e3, r


def inputs():
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    return model, proj, depth, synth.hypotheses(256)


def grid_of(nn, mm):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        g = api.Scene_grid.from_scene_nn(nn, mm * 1e-3)
    return g, bool(caught)


def scenes(depth, cells):
    out = {"a_projective": api.Scene_projective().init_Scene_projective_cuda(depth, K), "b_kdtree": api.Scene_nn().init_Scene_nn_cuda(depth, K)}
    info = {}
    for mm in cells:
        g, shrunk = grid_of(out["b_kdtree"], mm)
        out[f"c_grid_{mm:g}mm"] = g
        info[f"c_grid_{mm:g}mm"] = {"dim": list(g.dim), "bytes": g.nbytes, "box_shrunk": shrunk}
    return out, info


def step_time(args, solve):
    api.set_option("solve", api.SOLVE_DEVICE if solve == "device" else api.SOLVE_HOST)
    model, proj, depth, poses = inputs()
    sc, info = scenes(depth, args.cells)
    crit = api.ICPConvergenceCriteria(*CRIT)
    r = interleaved({k: (lambda s=s: api.refine_batch(model, poses, W, H, proj, K, s, crit)) for k, s in sc.items()}, args.calls, args.warmup)
    for k in r:
        r[k]["poses_per_s"] = round(256.0 / (r[k]["median_ms"] * 1e-3), 1)
        r[k].update(info.get(k, {}))
    return {"solve": solve, "calls": args.calls, "warmup_calls": args.warmup, "cases": r}


def step_build(args):
    model, proj, obj, _ = inputs()
    yy, xx = np.mgrid[0:H, 0:W]
    wall = (900 + 0.05 * xx + 0.03 * yy + 3.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)).astype(np.int32)       # tools/scene_frame_time.py's frame-filling scene
    out = {}
    for name, depth in (("object_alone", obj.astype(np.int32)), ("object_and_wall", np.where(obj > 0, obj, wall).astype(np.int32))):
        dev = api.DeviceVector.from_host(depth.reshape(-1))
        nn = api.Scene_nn()
        prep = [timed(lambda: nn.init_Scene_nn_device(dev, K, W, H))[0] for _ in range(args.warmup + 5)][args.warmup:]
        r = {"points": int((depth > 0).sum()), "kdtree_prepare_dev": stats(prep)}
        lib, C = api._lib.load(), api.C
        for mm in args.cells:
            g, shrunk = grid_of(nn, mm)                           # (also derives the tree's traversal records: not part of the build timed below)
            d, n = g.desc(), nn.desc()
            ms = [timed(lambda: api.check(lib.pr_scene_grid_build_dev(C.addressof(n), C.addressof(d), g.cell_buffer.data(), g.rec_buffer.data())))[0]
                  for _ in range(args.warmup + 5)][args.warmup:]
            cp = g.cell_points()
            r[f"grid_{mm:g}mm"] = {"build": stats(ms), "dim": list(g.dim), "cells": int(cp.size), "bytes": g.nbytes, "box_shrunk": shrunk,
                                   "cells_with_a_point": int((cp != api._lib.GRID_NONE).sum())}
            del g, cp
        out[name] = r
    return out


def step_kernel(args):
    api.set_option("solve", api.SOLVE_DEVICE)
    model, proj, depth, poses = inputs()
    sc, _ = scenes(depth, args.cells)
    crit = api.ICPConvergenceCriteria(*CRIT)
    out = {}
    for k, s in sc.items():
        for _ in range(args.warmup):
            api.refine_batch(model, poses, W, H, proj, K, s, crit)
        api.set_option("profile", 1)
        try:
            api.profile_reset()
            for _ in range(5):
                api.refine_batch(model, poses, W, H, proj, K, s, crit)
            p = api.profile_read()
        finally:
            api.set_option("profile", 0)
        n = max(1, p["icp_launches"])
        out[k] = {"timed_batches": 5, "pass_launches": int(p["icp_launches"]), "pass_ms_per_batch": round(p["icp_kernel_ms"] / 5, 4),
                  "pass_us_per_launch": round(p["icp_kernel_ms"] * 1e3 / n, 3), "points_per_batch": int(p["icp_points"] // 5),
                  "render_ms_per_batch": round(p["render_ms"] / 5, 4), "cloud_ms_per_batch": round(p["cloud_ms"] / 5, 4)}
    return {"solve": "device", "note": "a kd-tree pass is four kernels inside one timed launch; a timed batch runs as one pose group", "cases": out}


def diameter(v):
    v = np.asarray(v, np.float64)
    sq = (v * v).sum(1)
    best = 0.0
    for i in range(0, len(v), 1024):
        best = max(best, float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v[i:i + 1024] @ v.T)).max()))
    return float(np.sqrt(best))


def step_accuracy(args):
    api.set_option("solve", api.SOLVE_DEVICE)
    model, proj, depth, poses = inputs()
    sc, _ = scenes(depth, args.cells)
    crit = api.ICPConvergenceCriteria(*CRIT)
    gt, diam = synth.scene_pose(), diameter(model.vertices)
    refined, out = {}, {"diameter_mm": round(diam, 3)}
    for k, s in sc.items():
        rec, _ = api.refine_batch(model, poses, W, H, proj, K, s, crit)
        refined[k] = api.refined_poses(rec, poses)
        d = api.pose_distance(model, refined[k], gt, None, K)
        add, mssd = api.mean_displacement(d), api.max_displacement(d)
        out[k] = {"add_below_0.1_diameter": int((add < 0.1 * diam).sum()), "mssd_below_1mm": int((mssd < 1.0).sum()), "add_mm_median": round(float(np.median(add)), 4),
                  "fitness_at_least_0.9": int((rec["fitness"] >= 0.9).sum())}
    for k in refined:
        if k.startswith("c_"):
            mssd = api.max_displacement(api.pose_distance(model, refined[k], refined["b_kdtree"]))
            out[k]["mssd_mm_to_kdtree"] = {"max": round(float(mssd.max()), 4), "median": round(float(np.median(mssd)), 5), "below_1mm": int((mssd < 1.0).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=lambda s: [float(v) for v in s.split(",")], default=[1.0, 2.0, 4.0], help="cell sizes in mm")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    args = ap.parse_args()
    if args.step is None:                                          # the driver: every step a fresh process under `timeout`; no step is started after one that failed
        allr = {"workload": "configs[1] / [2]: 256 obj_06 hypotheses, 640x480, refine_batch at (0, 0, 20)"}
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(args.calls),
                   "--warmup", str(args.warmup), "--cells", ",".join(f"{c:g}" for c in args.cells)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                print(json.dumps({"step": step, "failed": p.returncode, "stderr": p.stderr[-2000:]}), flush=True)
                sys.exit(1)
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            allr[step] = json.loads(line)[step]
        print(json.dumps(allr), flush=True)
        return
    api.init(0)
    fn = {"time-device": lambda: step_time(args, "device"), "time-host": lambda: step_time(args, "host"), "build": lambda: step_build(args),
          "kernel": lambda: step_kernel(args), "accuracy": lambda: step_accuracy(args)}[args.step]
    print(json.dumps({args.step: fn()}), flush=True)


if __name__ == "__main__":
    main()
