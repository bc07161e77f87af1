#!/usr/bin/env python3
"""Scene segments on the two-object table frame: what the stage costs, what it is small against, and what the voting finds on one segment.

The frame of tests/test_segments_gpu.py's scenario: obj_06 at synth.scene_pose() and the bumped blob, 640x480, over an analytic table tilted 25
degrees; api.PlaneParams and api.PPFModel at their defaults, api.SegmentParams(jump_mm=20).

  --reference   no GPU: the numpy restatements alone (tests/planes' host twin for the plane, tests/segments_ref.py, tests/ppf_ref.py) -- the
                share of each object's mask its largest segment holds and the rank of the first hypothesis with ADD < 0.1 d on obj_06's segment:
                the constants OBJECT_SHARE_REF and E2E_N of the test come from here.
  default       on the device: host clock around the synchronous calls, the calls of one round interleaved, median / min / max of --calls after
                --warmup: scene_segments on the scenario's cleared frame next to scene_planes and init_Scene_projective_device on the same frame,
                and scene_segments on the 640x480 spiral, noise and constant frames (a labelling's time depends on content).
  --one-call    the calls once each, for a kernel trace taken around this script (the per-kernel times of profiles/segments/README.md).
Prints one JSON line; --write FILE also stores it (profiles/segments/README.md quotes the stored lines).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
import segments_cases as SC  # noqa: E402
import segments_ref as R  # noqa: E402


SCENARIO_JUMP_MM = 20        # the scenario's link threshold: at the default 10 the reference cuts obj_06 in two (profiles/segments/README.md)

CONTENT_MIN_PIXELS = 2       # the 640x480 noise frame has 83 739 components, 1-pixel ones included: over PR_SEGMENT_MAX_ROOTS at min_pixels = 1


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def diameter(v):
    v64 = np.asarray(v, np.float64)
    sq = (v64 * v64).sum(1)
    return math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))


def add_of(poses, gt, verts):
    v = np.asarray(verts, np.float64)
    out = []
    for T in np.asarray(poses, np.float64).reshape(-1, 4, 4):
        d = (T - np.asarray(gt, np.float64))[:3]
        out.append(float(np.sqrt(((v @ d[:, :3].T + d[:, 3]) ** 2).sum(1)).mean()))
    return np.array(out)


def scenario_frame():
    """the frame from the oracle's renders (bit-identical to the library's), on the CPU"""
    import oracle_lib as O
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    proj = O.compute_proj(K, W, H)
    tris = O.ply_load(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    blob_tris, blob_pose = SC.blob_mesh_and_pose()
    d_obj = O.render(tris, synth.scene_pose()[None], W, H, proj)[0]
    d_blob = O.render(blob_tris, blob_pose[None], W, H, proj)[0]
    depth, m_obj, m_blob = SC.two_object_frame(d_obj, d_blob)
    return tris, depth, m_obj, m_blob


def reference(jump_mm):
    import oracle_lib as O
    import ppf_ref as P
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    tris, depth, m_obj, m_blob = scenario_frame()
    full = O.ProjScene(depth, K)
    planes, plab, cleared = api.scene_planes_host(full.pcd, full.normal, depth, W, H)
    sp = api.SegmentParams(jump_mm=jump_mm)
    ref = R.scene_segments(cleared, sp.jump_mm, sp.min_pixels, sp.max_segments)
    lab = ref["labels"]
    k_obj, share_obj = SC.largest_share(lab, m_obj)
    k_blob, share_blob = SC.largest_share(lab, m_blob)
    both = sorted(set(lab[m_obj].tolist()) & set(lab[m_blob].tolist()) - {0, R.SEGMENT_DROPPED})
    out = {"jump_mm": jump_mm, "planes": len(planes), "object_pixels": int(m_obj.sum()), "blob_pixels": int(m_blob.sum()), "counts": ref["counts"],
           "segment_pixels": ref["segments"]["pixels"].tolist(), "obj_label": k_obj, "obj_share": share_obj, "blob_label": k_blob, "blob_share": share_blob,
           "labels_in_both_masks": both}
    kept = R.segment_depth(lab, cleared, k_obj)
    sc = O.ProjScene(kept, K)
    spts, snrm = P.scene_points(sc.pcd, sc.normal, W, H, 4)
    pm = api.PPFModel(tris)
    hyp, votes = P.hypotheses(P.tables(pm.params), pm.points, pm.normals, spts, snrm, 5, pm.dist_step_mm)
    verts = tris.reshape(-1, 3)
    diam = diameter(np.unique(verts, axis=0))
    add = add_of(hyp, synth.scene_pose(), verts)
    good = np.flatnonzero(add < 0.1 * diam)
    out["ppf_ref"] = {"scene_points": len(spts), "hypotheses": len(hyp), "diameter": diam, "first_correct_rank": int(good[0]) + 1 if len(good) else None,
                      "add_first": float(add[0]) if len(add) else None, "correct": int(len(good))}
    return out


def timed(calls, n_calls, warmup):
    ms = {k: [] for k in calls}
    for it in range(warmup + n_calls):                            # interleaved: every call sees the same state of the machine
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if it >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def content_frames():
    sp = np.where(SC.spiral_mask(640, 480), 900, 0).astype(np.uint16)
    return {"spiral_640x480": sp, "noise_640x480": SC.noise(640, 480, seed=3).astype(np.uint16), "constant_640x480": np.full((480, 640), 900, np.uint16)}


def device(args):
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    tris, depth, m_obj, m_blob = scenario_frame()
    depth_dev = api.DeviceVector.from_host(depth.reshape(-1))
    full = api.Scene_projective().init_Scene_projective_device(depth_dev, K, W, H)
    pp, sp = api.PlaneParams(), api.SegmentParams(jump_mm=args.jump_mm)
    planes, plab, cleared = api.scene_planes(full, depth_dev, params=pp)
    segs, labels, counts = api.scene_segments(cleared, W, H, params=sp)
    lab = labels.to_host().reshape(H, W)
    out = {"workload": "obj_06.ply at synth.scene_pose() and the bumped blob on a table tilted 25 degrees, 640x480, PlaneParams defaults, SegmentParams(jump_mm)",
           "jump_mm": args.jump_mm, "calls": args.calls, "warmup_calls": args.warmup, "counts": counts, "segment_pixels": segs["pixels"].tolist(),
           "obj_share": SC.largest_share(lab, m_obj)[1], "blob_share": SC.largest_share(lab, m_blob)[1]}
    if args.one_call:                                              # the call a kernel trace is taken of: the scenario, then the spiral and the noise frame
        for name, fr in content_frames().items():
            api.scene_segments(api.DeviceVector.from_host(fr.reshape(-1)), 640, 480, min_pixels=CONTENT_MIN_PIXELS, max_segments=R.SEGMENT_MAX)
        return out
    scratch = api.Scene_projective()
    calls = {"scene_segments": lambda: api.scene_segments(cleared, W, H, params=sp),
             "scene_planes": lambda: api.scene_planes(full, depth_dev, params=pp),
             "init_Scene_projective_device": lambda: scratch.init_Scene_projective_device(cleared, K, W, H),
             "segment_depth": lambda: api.segment_depth(labels, cleared, 1)}
    frames = {k: api.DeviceVector.from_host(v.reshape(-1)) for k, v in content_frames().items()}
    out["content_counts"] = {}
    for name, fr in frames.items():
        calls["scene_segments_" + name] = (lambda fr=fr: api.scene_segments(fr, 640, 480, min_pixels=CONTENT_MIN_PIXELS, max_segments=R.SEGMENT_MAX))
        out["content_counts"][name] = api.scene_segments(fr, 640, 480, min_pixels=CONTENT_MIN_PIXELS, max_segments=R.SEGMENT_MAX)[-1]
    out["time_ms"] = timed(calls, args.calls, args.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jump-mm", type=int, default=SCENARIO_JUMP_MM)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--write", default=None)
    args = ap.parse_args()
    out = reference(args.jump_mm) if args.reference else device(args)
    line = json.dumps(out)
    print(line, flush=True)
    if args.write:
        os.makedirs(os.path.dirname(os.path.abspath(args.write)), exist_ok=True)
        with open(args.write, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
