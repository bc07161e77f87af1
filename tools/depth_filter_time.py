#!/usr/bin/env python3
"""Depth conditioning at 640x480: what depth_fuse and depth_filter cost, what they are small against, and what the stages behind them make of a
corrupted frame with and without conditioning.

The frame of tools/segments_time.py (obj_06 at synth.scene_pose() and the bumped blob over the table tilted 25 degrees), corrupted by the recipe
of tests/depth_filter_ref.py (noise in -2 .. 2, flying pixels at depth jumps of more than 60 mm, 2 % holes and one 3 x 3 hole), seeds 0 .. 4.

  default   on the device: host clock around the synchronous calls, the calls of one round interleaved, median / min / max of --calls after
            --warmup: depth_fuse of the five frames and depth_filter at radius 1 and 2, both depth types, next to segment_depth and
            init_Scene_projective_device on the same frame; then the scenario on frame 0 as it is and conditioned (fuse of the five, then filter):
            scene_planes' angle and offset error against the analytic table, the number of scene_segments and the share of obj_06's mask its
            largest segment holds, the rank of the first generate_hypotheses hypothesis with ADD < 0.1 d, score_poses' counts for the true pose.
  --one-call  ten rounds of the timed calls and nothing else, for a kernel trace taken around this script (the per-kernel times of
            profiles/depth_filter/README.md).
Prints one JSON line; --write FILE also stores it (profiles/depth_filter/README.md quotes the stored lines).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
import depth_filter_ref as R  # noqa: E402
import planes_cases as PC  # noqa: E402
import segments_cases as SC  # noqa: E402
import segments_time as ST  # noqa: E402

PARAMS = dict(min_mm=100, max_mm=2000, tol_mm=8, tol_permille=5, fly_min_support=3)
WINDOWS = {"r1": dict(radius=1, fill_min=5), "r2": dict(radius=2, fill_min=13)}
TAU_MM = 5


def table_plane(depth, both):
    """the analytic table of SC.two_object_frame: (unit normal, offset) with normal . p + offset = 0"""
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    n = PC.tilted(SC.TABLE_TILT_DEG)
    den = PC.rays(W, H, K) @ n
    return n, -(math.ceil((depth[both].astype(np.float64) * np.abs(den[both])).max()) + 5.0)


def scenario(tag, depth_dev, model, pm, m_obj, n_true, d_true, diam):
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    proj, gt = api.compute_proj(K, W, H), synth.scene_pose()
    out = {}
    full = api.Scene_projective().init_Scene_projective_device(depth_dev, K, W, H)
    planes, _, cleared = api.scene_planes(full, depth_dev)
    out["planes"] = len(planes)
    if len(planes):
        n = planes[0]["normal"].astype(np.float64)
        out["plane_angle_deg"] = round(math.degrees(math.acos(min(1.0, abs(float(n @ n_true)) / float(np.linalg.norm(n))))), 4)
        out["plane_offset_err_mm"] = round(abs(abs(float(planes[0]["offset_mm"])) - abs(d_true)), 3)
        out["plane_rms_mm"] = round(float(planes[0]["rms_mm"]), 3)
    segs, labels, counts = api.scene_segments(cleared, W, H, jump_mm=ST.SCENARIO_JUMP_MM)
    lab = labels.to_host().reshape(H, W)
    k_obj, share = SC.largest_share(lab, m_obj)
    out["segments"] = counts
    out["obj_share"] = round(share, 5)
    if k_obj:
        kept = api.segment_depth(labels, cleared, k_obj)
        scene = api.Scene_projective().init_Scene_projective_device(kept, K, W, H)
        hyp, votes = api.generate_hypotheses(pm, scene)
        add = api.mean_displacement(api.pose_distance(model, hyp, gt)) if len(hyp) else np.zeros(0)
        good = np.flatnonzero(add < 0.1 * diam)
        out["hypotheses"] = len(hyp)
        out["first_correct_rank"] = int(good[0]) + 1 if len(good) else None
    s = api.score_poses(model, gt[None], W, H, proj, depth_dev, TAU_MM)[0]
    out["score_true_pose"] = {k: int(s[k]) for k in ("visible", "inlier", "occluded", "violation", "missing")}
    return out


def device(args):
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    tris, clean, m_obj, m_blob = ST.scenario_frame()
    n_true, d_true = table_plane(clean, m_obj | m_blob)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    diam = ST.diameter(np.unique(tris.reshape(-1, 3), axis=0))
    frames = [R.corrupt(clean.astype(np.int64), seed, hole_block=((160, 163), (200, 203))) for seed in range(5)]
    out = {"workload": "obj_06 and the blob on the 25-degree table, 640x480, corrupted (noise -2 .. 2, flying pixels at jumps > 60 mm, 2 % holes), seeds 0 .. 4",
           "params": PARAMS, "windows": WINDOWS, "calls": args.calls, "warmup_calls": args.warmup,
           "injected": {"flying": [int(f[1].sum()) for f in frames], "holes": [int(f[2].sum()) for f in frames]}}
    calls, scratch = {}, api.Scene_projective()
    for dtype in (np.uint16, np.int32):
        name = np.dtype(dtype).name
        dev = [api.DeviceVector.from_host(f[0].astype(dtype).reshape(-1)) for f in frames]
        fused, filtered = api.DeviceVector(W * H, dtype), api.DeviceVector(W * H, dtype)
        calls[f"depth_fuse_5_{name}"] = (lambda dev=dev, fused=fused: api.depth_fuse(dev, W, H, min_frames=3, depth_out=fused))
        for wname, win in WINDOWS.items():
            dp = api.DepthFilterParams(**PARAMS, **win)
            calls[f"depth_filter_{wname}_{name}"] = (lambda dev=dev, dp=dp, filtered=filtered: api.depth_filter(dev[0], W, H, params=dp, depth_out=filtered))
        if dtype == np.uint16:
            labels = api.scene_segments(dev[0], W, H, jump_mm=ST.SCENARIO_JUMP_MM)[1]
            calls["segment_depth"] = (lambda dev=dev, labels=labels, filtered=filtered: api.segment_depth(labels, dev[0], 1, depth_out=filtered))
            calls["init_Scene_projective_device"] = (lambda dev=dev: scratch.init_Scene_projective_device(dev[0], K, W, H))
            keep = dev
    if args.one_call:                                              # the calls a kernel trace is taken of: ten of each, nothing else
        ST.timed(calls, 10, 0)
        return out
    out["time_ms"] = ST.timed(calls, args.calls, args.warmup)
    # the scenario: one corrupted frame as it is, the same frame filtered, and the five fused and filtered
    pm = api.PPFModel(model)
    dp = api.DepthFilterParams(**PARAMS, **WINDOWS["r1"])
    one, flags, counts = api.depth_filter(keep[0], W, H, params=dp, want_flags=True)
    fl = flags.to_host().reshape(H, W)
    out["filter_counts_frame0"] = counts
    out["flying_removed"] = round(float((fl[frames[0][1]] == api.DEPTH_FLYING).mean()), 4)
    fused = api.depth_fuse(keep, W, H, min_frames=3)
    both, counts_fused = api.depth_filter(fused, W, H, params=dp)
    out["filter_counts_fused"] = counts_fused
    clean_dev = api.DeviceVector.from_host(clean.astype(np.uint16).reshape(-1))
    for tag, d in (("clean", clean_dev), ("corrupted", keep[0]), ("filtered", one), ("fused_filtered", both)):
        out["scenario_" + tag] = scenario(tag, d, model, pm, m_obj, n_true, d_true, diam)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--write", default=None)
    args = ap.parse_args()
    out = device(args)
    line = json.dumps(out)
    print(line, flush=True)
    if args.write:
        os.makedirs(os.path.dirname(os.path.abspath(args.write)), exist_ok=True)
        with open(args.write, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
