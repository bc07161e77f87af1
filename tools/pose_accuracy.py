#!/usr/bin/env python
"""How many refined hypotheses end at the right pose, in pose-error terms, and what measuring that costs.  On configs[1] (projective scene)
and configs[2] (kd-tree scene), the 256 synth hypotheses of obj_06 at 640x480 against the known scene pose (synth.scene_pose()):
  unrefined, refine_batch at (0, 0, 20), refine_pyramid(PYRAMID_DEFAULT)  ->  ADD / MSSD / MSPD (api.pose_distance over the model's
  15 736 vertices, no symmetries: obj_06 has none): median, maximum, how many have ADD < 0.1 x the model diameter and MSSD < 1 mm;
  merge_duplicates at 1 mm in rank_hypotheses' order (score_poses, tau 5): how many distinct poses the batch holds;
  the pyramid against refine_batch hypothesis by hypothesis (over those refine_batch converges on, fitness >= 0.9);
  VSD (api.pose_vsd against the scene's depth frame, BOP's delta of 15 mm and taus of 0.05 .. 0.5 x the diameter, with K): the median error at
  tau = 0.2 d, the recall over taus and thresholds (api.vsd_recall), the MSSD and MSPD recalls over BOP's thresholds (0.05 .. 0.5 x the diameter;
  5 .. 50 px at 640 px width) and the mean of the three -- the field's average recall, for one object in one frame.
Then the time of pose_distance (256 pairs) and pose_distance_matrix (256 x 256), each with and without K: host clocks around the synchronous
calls, after warm-up, the four cases interleaved call by call; median / min / max ms.  One JSON line.

    python tools/pose_accuracy.py [--calls 30] [--warmup 5] [--solve device|host]
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


def diameter(v):
    """Largest distance between two vertices, float64, by blocks of rows."""
    v = np.asarray(v, np.float64)
    sq = (v * v).sum(1)
    best = 0.0
    for i in range(0, len(v), 1024):
        d2 = sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v[i:i + 1024] @ v.T)
        best = max(best, float(d2.max()))
    return float(np.sqrt(best))


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


def errors(model, poses, gt, K, diam, frame):
    d = api.pose_distance(model, poses, gt, None, K)
    add, mssd, mspd = api.mean_displacement(d), api.max_displacement(d), api.max_projection(d)
    r3 = lambda x: round(float(x), 4)  # noqa: E731
    W, H, proj, depth_dev = frame
    taus = [t * diam for t in api.VSD_TAUS_BOP]
    ve = api.vsd_errors(api.pose_vsd(model, poses, gt, W, H, proj, depth_dev, K, api.VSD_DELTA_BOP, taus), len(taus))
    th = np.asarray(api.VSD_THRESHOLDS_BOP)
    ar_vsd, ar_mssd = api.vsd_recall(ve), float((mssd[:, None] < th * diam).mean())
    ar_mspd = float((mspd[:, None] < np.arange(5, 51, 5) * (W / 640.0)).mean())
    return {"vsd_error_at_0.2_diameter_median": r3(np.median(ve[:, api.VSD_TAUS_BOP.index(0.2)])), "recall_vsd": r3(ar_vsd), "recall_mssd": r3(ar_mssd),
            "recall_mspd": r3(ar_mspd), "recall_mean": r3((ar_vsd + ar_mssd + ar_mspd) / 3.0),
            "add_mm": {"median": r3(np.median(add)), "max": r3(add.max())}, "mssd_mm": {"median": r3(np.median(mssd)), "max": r3(mssd.max())},
            "mspd_px": {"median": r3(np.median(mspd)), "max": r3(mspd.max())},
            "add_below_0.1_diameter": int((add < 0.1 * diam).sum()), "mssd_below_1mm": int((mssd < 1.0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--solve", choices=["device", "host"], default="device")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE if args.solve == "device" else api.SOLVE_HOST)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    depth = api.render_host(model, gt[None], W, H, proj)[0]
    poses = synth.hypotheses(256)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    diam = diameter(model.vertices)
    frame = (W, H, proj, api.DeviceVector.from_host(depth.reshape(-1)))
    out = {"workload": "configs[1] / configs[2]: obj_06.ply (15736 vertices), 256 synth hypotheses, 640x480, against synth.scene_pose(); no symmetries",
           "solve": args.solve, "diameter_mm": round(diam, 3), "schedule": [[s, list(c)] for s, c in api.PYRAMID_DEFAULT],
           "unrefined": errors(model, poses, gt, K, diam, frame)}
    refined_proj = None
    for kind in ("proj", "nn"):
        scene = api.Scene_projective().init_Scene_projective_cuda(depth, K) if kind == "proj" else api.Scene_nn().init_Scene_nn_cuda(depth, K)
        a, _ = api.refine_batch(model, poses, W, H, proj, K, scene, crit)
        b, _ = api.refine_pyramid(model, poses, W, H, proj, K, scene, api.PYRAMID_DEFAULT)
        r = {}
        sets = {"refine_batch_20": api.refined_poses(a, poses), "refine_pyramid": api.refined_poses(b, poses)}
        for name, ref in sets.items():
            e = errors(model, ref, gt, K, diam, frame)
            order = api.rank_hypotheses(api.score_poses(model, ref, W, H, proj, depth, 5))
            kept, _ = api.merge_duplicates(order, api.pose_distance_matrix(model, ref), 1.0)
            e["distinct_at_1mm"] = int(len(kept))
            r[name] = e
        ok = a["fitness"] >= 0.9
        d = api.pose_distance(model, sets["refine_pyramid"], sets["refine_batch_20"])
        add, mssd = api.mean_displacement(d), api.max_displacement(d)
        r["pyramid_vs_batch_converged"] = {"converged_batch": int(ok.sum()), "mssd_within_0.05mm": int((mssd[ok] <= 0.05).sum()),
                                           "add_within_0.05mm": int((add[ok] <= 0.05).sum()), "mssd_mm_max": round(float(mssd[ok].max()), 4),
                                           "mssd_mm_median": round(float(np.median(mssd[ok])), 5),
                                           "mssd_above_1mm": int((mssd[ok] > 1.0).sum())}
        out[kind] = r
        if kind == "proj":
            refined_proj = sets["refine_batch_20"]
    model.device_vertices()
    t = interleaved({"pairs_256": lambda: api.pose_distance(model, refined_proj, gt),
                     "pairs_256_K": lambda: api.pose_distance(model, refined_proj, gt, None, K),
                     "matrix_256x256": lambda: api.pose_distance_matrix(model, refined_proj),
                     "matrix_256x256_K": lambda: api.pose_distance_matrix(model, refined_proj, None, None, K)}, args.calls, args.warmup)
    t["calls"], t["warmup_calls"] = args.calls, args.warmup
    t["candidate_points_matrix"] = 256 * 256 * len(model.vertices)
    out["time"] = t
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
