#!/usr/bin/env python3
"""Point-pair-feature voting on the flagship frame: what it costs and what it finds.

obj_06 at synth.scene_pose(), 640x480, the library's own render as the frame; api.PPFModel with its defaults, stride 4, ref_stride 5.
Times (host clock around the synchronous calls, median of --calls after --warmup): the model build (pr_ppf_model_build_dev), the scene sample
(pr_ppf_scene_points_dev), pr_ppf_vote with either bucket walk (option "ppf_walk", alternating) and with 4 peaks, api.generate_hypotheses whole, and the refine_batch call that consumes the list.
Accuracy, from the frame alone (no supplied poses): how many of the first 256 hypotheses have ADD < 0.1 x the model diameter before and after
refine_batch (projective and kd-tree scene, 20 iterations), the rank of the first such hypothesis, and the MSSD of the hypothesis ICP rates best.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
from pose_accuracy import diameter, stats  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--ref-stride", type=int, default=5)
    args = ap.parse_args()
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    depth = api.render_host(model, gt[None], W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    scene_nn = api.Scene_nn().init_Scene_nn_cuda(depth, K)
    diam = diameter(model.vertices)
    pm = api.PPFModel(model).build()
    pts, nrm, n_scene = api.ppf_scene_points(scene, args.stride)
    n_refs = (n_scene - 1) // args.ref_stride + 1
    out = {"workload": "obj_06.ply at synth.scene_pose(), 640x480, PPFModel defaults", "diameter_mm": round(diam, 3), "step_mm": round(pm.step_mm, 4),
           "n_model": len(pm.points), "n_keys": pm.params.n_keys, "n_entries": pm.n_entries, "stride": args.stride, "ref_stride": args.ref_stride,
           "n_scene": n_scene, "n_refs": n_refs, "calls": args.calls, "warmup_calls": args.warmup}

    def rebuild():
        pm.offsets = None
        pm.build()
    peaks, _ = api.ppf_vote(pm, pts, nrm, n_scene, 0, args.ref_stride, n_refs, 1)
    out["peak_votes"] = int(peaks["votes"].astype(np.int64).sum())          # the votes of the 276 peaks (the accumulators hold more)
    out["pairs"] = int(peaks["n_pairs"].astype(np.int64).sum())
    vote = {}                                # the two bucket walks (option "ppf_walk"), alternating call by call; the same peaks from both
    walks = (("vote_1_peak_lane_walk", 0), ("vote_1_peak_wave_walk", 1))
    ms = {k: [] for k, _ in walks}
    for it in range(args.warmup + args.calls):
        for k, w in walks:
            api.set_option("ppf_walk", w)
            t0 = time.perf_counter()
            vote[k] = api.ppf_vote(pm, pts, nrm, n_scene, 0, args.ref_stride, n_refs, 1)
            if it >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    assert vote[walks[0][0]][0].tobytes() == vote[walks[1][0]][0].tobytes() == peaks.tobytes()
    api.set_option("ppf_walk", 1)
    walk_ms = {k: stats(v) for k, v in ms.items()}
    out["time_ms"] = {"model_build": timed(rebuild, args.calls, args.warmup),
                      "scene_sample": timed(lambda: api.ppf_scene_points(scene, args.stride), args.calls, args.warmup),
                      "vote_4_peaks": timed(lambda: api.ppf_vote(pm, pts, nrm, n_scene, 0, args.ref_stride, n_refs, 4), args.calls, args.warmup),
                      "generate_hypotheses": timed(lambda: api.generate_hypotheses(pm, scene, args.stride, args.ref_stride), args.calls, args.warmup)}
    out["time_ms"].update(walk_ms)
    hyp, votes = api.generate_hypotheses(pm, scene, args.stride, args.ref_stride)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    out["time_ms"]["refine_batch_proj_20"] = timed(lambda: api.refine_batch(model, hyp, W, H, proj, K, scene, crit), args.calls, args.warmup)
    add = api.mean_displacement(api.pose_distance(model, hyp, gt))
    good = np.flatnonzero(add < 0.1 * diam)
    out["hypotheses"] = {"count": len(hyp), "add_below_0.1_diameter": int(len(good)), "first_correct_rank": int(good[0]) + 1 if len(good) else None,
                         "add_mm_median": round(float(np.median(add)), 3), "add_mm_best": round(float(add.min()), 3), "votes_first": int(votes[0])}
    for kind, sc in (("proj", scene), ("nn", scene_nn)):
        res, _ = api.refine_batch(model, hyp, W, H, proj, K, sc, crit)
        d = api.pose_distance(model, api.refined_poses(res, hyp), gt)
        a, m = api.mean_displacement(d), api.max_displacement(d)
        best = int(np.lexsort((res["inlier_rmse"], -res["fitness"]))[0])
        out["refined_" + kind] = {"add_below_0.1_diameter": int((a < 0.1 * diam).sum()), "mssd_below_1mm": int((m < 1.0).sum()), "best_by_fitness": best,
                                  "best_mssd_mm": round(float(m[best]), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
