#!/usr/bin/env python
"""What coarse-to-fine refinement costs against full-resolution refinement, on configs[1]: 256 obj_06 hypotheses, 640x480, projective scene,
device solve (host clocks around synchronous calls, after warm-up; the three cases INTERLEAVED call by call in one process):
  (a) refine_batch at (0, 0, 20);
  (b) refine_pyramid(PYRAMID_DEFAULT);
  (c) refine_pyramid with one stride-1 level of 20 iterations -- (c) - (a) is the cost of the new plumbing (the synchronous level loop
      against the asynchronous slot refine_batch runs on).
The same three on the kd-tree scene.  One JSON line: median / min / max ms per case, max |dt| of (b) against (a) over the hypotheses
whose (a) fitness is >= 0.9 (maximum, median, how many within 0.05 mm; the maximum over those (b) converges on as well), the point-passes of (b) as a fraction of (a)'s, and whether median (b) is below min (a).

    python tools/pyramid_time.py [--calls 50] [--nn-calls 20] [--warmup 5] [--solve device|host] [--only b] [--scene proj|nn]

--only a|b|c runs just that case on --scene (a profiler run of one case).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pose_refine_amd import api, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--nn-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--solve", choices=["device", "host"], default="device")
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--scene", choices=["proj", "nn"], default="proj")
    args = ap.parse_args()
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE if args.solve == "device" else api.SOLVE_HOST)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    obj = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(obj, synth.scene_pose()[None], W, H, proj)[0]
    poses = synth.hypotheses(256)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    full = [api.PyramidLevel(1, crit)]

    def cases(scene):
        return {"a": lambda: api.refine_batch(obj, poses, W, H, proj, K, scene, crit),
                "b": lambda: api.refine_pyramid(obj, poses, W, H, proj, K, scene, api.PYRAMID_DEFAULT),
                "c": lambda: api.refine_pyramid(obj, poses, W, H, proj, K, scene, full)}

    def make(kind):
        return api.Scene_projective().init_Scene_projective_cuda(depth, K) if kind == "proj" else api.Scene_nn().init_Scene_nn_cuda(depth, K)

    out = {"workload": "configs[1]: 256 obj_06 hypotheses, 640x480; (a) refine_batch 20 iterations, (b) refine_pyramid(PYRAMID_DEFAULT), (c) refine_pyramid, one stride-1 level of 20",
           "solve": args.solve, "schedule": [[s, list(c)] for s, c in api.PYRAMID_DEFAULT], "warmup_calls": args.warmup}
    if args.only:
        fn = cases(make(args.scene))[args.only]
        out[args.scene] = interleaved({args.only: fn}, args.calls, args.warmup)
        out["calls"] = args.calls
        print(json.dumps(out), flush=True)
        return
    for kind, calls in (("proj", args.calls), ("nn", args.nn_calls)):
        scene = make(kind)
        c = cases(scene)
        r = interleaved(c, calls, args.warmup)
        r["calls"] = calls
        r["c_minus_a_median_ms"] = round(r["c"]["median_ms"] - r["a"]["median_ms"], 4)
        r["median_b_below_min_a"] = bool(r["b"]["median_ms"] < r["a"]["min_ms"])
        a, asz = c["a"]()
        b, blr, bsz = api.refine_pyramid(obj, poses, W, H, proj, K, scene, api.PYRAMID_DEFAULT, return_levels=True)
        one = c["c"]()
        ok = a["fitness"] >= 0.9
        dt = np.linalg.norm(b["T"].reshape(-1, 4, 4)[:, :3, 3].astype(np.float64) - a["T"].reshape(-1, 4, 4)[:, :3, 3].astype(np.float64), axis=1) * 1e3
        r["converged_a"] = int(ok.sum())
        r["max_dt_mm_b_vs_a_converged"] = round(float(dt[ok].max()), 5) if ok.any() else None
        r["median_dt_mm_b_vs_a_converged"] = round(float(np.median(dt[ok])), 5) if ok.any() else None
        r["converged_a_within_0.05mm"] = int((dt[ok] <= 0.05).sum())
        r["converged_b"] = int((b["fitness"] >= 0.9).sum())
        both = ok & (b["fitness"] >= 0.9)
        r["converged_both"] = int(both.sum())
        r["max_dt_mm_converged_both"] = round(float(dt[both].max()), 5) if both.any() else None
        passes = np.array([[lv[1][2] + 1] for lv in api.PYRAMID_DEFAULT], np.float64)
        r["point_passes_b_over_a"] = round(float((bsz.astype(np.float64) * passes).sum() / (asz.astype(np.float64) * 21).sum()), 4)
        r["level_points_b"] = [int(x) for x in bsz.sum(axis=1)]
        r["c_equals_a_bytes"] = bool(one[0].tobytes() == a.tobytes() and np.array_equal(one[1], asz))
        out[kind] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
