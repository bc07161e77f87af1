#!/usr/bin/env python3
"""Support-plane removal on the table frame: what it costs, what it is small against, and what the voting finds with and without it.

obj_06 at synth.scene_pose(), 640x480, the library's own render over an analytic table (the plane z = const turned 25 degrees about the camera's
x axis, 5 mm behind the object pixel nearest to it), api.PlaneParams and api.PPFModel at their defaults.  Times (host clock around the synchronous
calls, the calls of one round interleaved, median / min / max of --calls after --warmup): pr_scene_planes_dev for 1 and 2 planes, and in the same
session pr_scene_proj_prepare_dev, pr_ppf_scene_points_dev and pr_ppf_vote on the cleared frame.  Accuracy from the frame alone: the plane
against the analytic one, the object pixels it takes, and the hypotheses of api.generate_hypotheses on the cleared frame (count, first rank with
ADD < 0.1 d); without removal: the refusal at stride 4 and the same figures at stride 8.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
from pose_accuracy import diameter, stats  # noqa: E402


def table_depth(render, K, W, H, tilt_deg=25.0, gap_mm=5.0):
    a = math.radians(tilt_deg)
    n = np.array([0.0, math.sin(a), -math.cos(a)])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    den = ((v - float(K[5])) / float(K[4])) * n[1] + n[2]
    obj = render > 0
    d = -(math.ceil((render[obj].astype(np.float64) * np.abs(den[obj])).max()) + gap_mm)
    return np.where(obj, render, np.rint(d / den)).astype(np.uint16), obj, n, d


def hypotheses_of(pm, scene, model, gt, diam, stride):
    hyp, votes = api.generate_hypotheses(pm, scene, stride)
    add = api.mean_displacement(api.pose_distance(model, hyp, gt))
    good = np.flatnonzero(add < 0.1 * diam)
    return {"stride": stride, "count": len(hyp), "add_below_0.1_diameter": int(len(good)), "first_correct_rank": int(good[0]) + 1 if len(good) else None,
            "votes_first": int(votes[0]) if len(votes) else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    depth, obj, n, d = table_depth(api.render_host(model, gt[None], W, H, proj)[0], K, W, H)
    depth_dev = api.DeviceVector.from_host(depth.reshape(-1))
    full = api.Scene_projective().init_Scene_projective_device(depth_dev, K, W, H)
    diam = diameter(model.vertices)
    pm = api.PPFModel(model).build()
    pp1, pp2 = api.PlaneParams(n_planes=1), api.PlaneParams(n_planes=2)
    planes, labels, cleared = api.scene_planes(full, depth_dev, params=pp1)
    lab = labels.to_host().reshape(H, W)
    nf = planes[0]["normal"].astype(np.float64)
    out = {"workload": "obj_06.ply at synth.scene_pose() on a table tilted 25 degrees, 640x480, PlaneParams and PPFModel defaults", "calls": args.calls,
           "warmup_calls": args.warmup, "stride": pp1.stride, "cand_stride": pp1.cand_stride,
           "plane": {"found": len(planes), "support": int(planes[0]["support"]), "labelled": int(planes[0]["labelled"]), "behind": int(planes[0]["behind"]),
                     "rms_mm": round(float(planes[0]["rms_mm"]), 4), "angle_deg": round(math.degrees(math.acos(min(1.0, float(nf @ n)))), 5),
                     "offset_error_mm": round(float(planes[0]["offset_mm"]) - d, 4), "object_pixels": int(obj.sum()),
                     "object_pixels_labelled": int((lab[obj] != 0).sum()), "table_pixels_left": int((lab[~obj] == 0).sum())}}
    scene = api.Scene_projective().init_Scene_projective_device(cleared, K, W, H)
    pts, nrm, n_scene = api.ppf_scene_points(scene, 4)
    n_refs = (n_scene - 1) // 5 + 1
    out["cleared"] = {"n_scene": n_scene, "n_refs": n_refs}
    scratch = api.Scene_projective()
    calls = {"scene_planes_1": lambda: api.scene_planes(full, depth_dev, params=pp1),
             "scene_planes_2": lambda: api.scene_planes(full, depth_dev, params=pp2),
             "scene_proj_prepare_dev": lambda: scratch.init_Scene_projective_device(cleared, K, W, H),
             "ppf_scene_points": lambda: api.ppf_scene_points(scene, 4),
             "ppf_vote_1_peak": lambda: api.ppf_vote(pm, pts, nrm, n_scene, 0, 5, n_refs, 1)}
    ms = {k: [] for k in calls}
    for it in range(args.warmup + args.calls):                    # interleaved: every call sees the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if it >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out["time_ms"] = {k: stats(v) for k, v in ms.items()}
    out["hypotheses_cleared"] = hypotheses_of(pm, scene, model, gt, diam, 4)
    try:
        api.ppf_scene_points(full, 4)
        out["without_removal_stride_4"] = "accepted"
    except api.PoseRefineError as e:
        out["without_removal_stride_4"] = f"refused (code {e.code})"
    out["n_scene_full_stride_8"] = api.ppf_scene_points(full, 8)[2]
    t0 = time.perf_counter()
    out["hypotheses_full_stride_8"] = hypotheses_of(pm, full, model, gt, diam, 8)
    out["hypotheses_full_stride_8"]["generate_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
