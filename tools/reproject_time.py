#!/usr/bin/env python3
"""Reprojection at a 640x480 target: what depth_reproject costs per call, next to depth_fuse of two frames and init_Scene_projective_device.

The frame of tools/segments_time.py (obj_06 at synth.scene_pose() and the bumped blob over the table tilted 25 degrees, 640 x 480, dense).  Sources:
that frame seen from a camera 60 mm to the side and turned 4 degrees; two such frames (the second from the other side); and the frame's own
depth2cloud cloud under the first transform.  Each at splat 1 and 2, without and with the visibility stage (occl_radius 1, occl_min_front 2).

  default   on the device: host clock around the synchronous calls, the calls of one round interleaved, median / min / max of --calls after
            --warmup, the outputs into vectors allocated before.
  --one-call  ten rounds of the timed calls and nothing else, for a kernel trace taken around this script (the per-kernel times of
            profiles/reproject/README.md).
Prints one JSON line; --write FILE also stores it (profiles/reproject/README.md quotes the stored line).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
import reproject_cases as RC  # noqa: E402
import segments_time as ST  # noqa: E402

VISIBILITY = dict(tol_mm=10, tol_permille=5, occl_radius=1, occl_min_front=2)


def device(args):
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    _, clean, _, _ = ST.scenario_frame()
    frame = api.DeviceVector.from_host(clean.astype(np.uint16).reshape(-1))
    other = api.DeviceVector.from_host(clean.astype(np.uint16).reshape(-1))
    cloud = api.depth2cloud(frame, W, H, K, dtype=np.uint16)
    T1, T2 = RC.rigid(ry=4.0, t=(-0.06, 0.0, 0.0)), RC.rigid(ry=-4.0, t=(0.06, 0.0, 0.0))
    sets = {"frame": [api.ReprojectSource.frame(frame, W, H, K, T1)],
            "two_frames": [api.ReprojectSource.frame(frame, W, H, K, T1), api.ReprojectSource.frame(other, W, H, K, T2)],
            "cloud": [api.ReprojectSource.cloud(cloud, T1)]}
    out = {"workload": "obj_06 and the blob on the 25-degree table, 640x480 uint16 into a 640x480 uint16 target", "measured_pixels": int((clean > 0).sum()),
           "cloud_points": cloud.size() // 3, "visibility": VISIBILITY, "calls": args.calls, "warmup_calls": args.warmup}
    dst, scratch, fused = api.DeviceVector(W * H, np.uint16), api.Scene_projective(), api.DeviceVector(W * H, np.uint16)
    calls, counts = {}, {}
    for sname, srcs in sets.items():
        for splat in (1, 2):
            for vname, vis in (("", {}), ("_vis", VISIBILITY)):
                rp = api.ReprojectParams(splat=splat, **vis)
                key = f"reproject_{sname}_s{splat}{vname}"
                calls[key] = (lambda srcs=srcs, rp=rp: api.depth_reproject(srcs, W, H, K, params=rp, depth_out=dst))
                c = calls[key]()[1]
                counts[key] = dict(drawn=[s["drawn"] for s in c["sources"]], covered=c["covered"], hidden=c["hidden"])
    calls["depth_fuse_2"] = (lambda: api.depth_fuse([frame, other], W, H, min_frames=1, depth_out=fused))
    calls["init_Scene_projective_device"] = (lambda: scratch.init_Scene_projective_device(frame, K, W, H))
    out["counts"] = counts
    if args.one_call:                                              # the calls a kernel trace is taken of: ten of each, nothing else
        ST.timed(calls, 10, 0)
        return out
    out["time_ms"] = ST.timed(calls, args.calls, args.warmup)
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
