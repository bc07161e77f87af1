#!/usr/bin/env python
"""What the contour check costs on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations), 640x480,
against the bench's int32 scene and a uint16 copy of it.  Per scene dtype, ms per call (median / min / max over --calls calls after
--warmup calls) of (a) pr_score_contours without the overlap matrix, (b) pr_score_poses on the same inputs, (c) pr_render_to_host of the
same poses -- the only route to the same information without (a), the host's edge tests not included -- and (d) pr_scene_edge_distance_dev,
once per frame.  One JSON line; `a_minus_b_ms` is the price of the contour records, `a_beats_c` says whether max(a) < min(c).

    python tools/contour_time.py [--calls 100] [--warmup 10] [--tau 5] [--jump 10] [--radius 3] [--only a|b|c|d]   (--only: one case, for a profiler run)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pose_refine_amd import _lib, api, synth  # noqa: E402
from select_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--jump", type=int, default=10)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b", "c", "d"])
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls: at least 50")
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    poses = synth.hypotheses(256)
    res, _ = api.refine_batch(model, poses, W, H, proj, K, scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = np.ascontiguousarray(api.refined_poses(res, poses).reshape(-1, 16))
    P = len(refined)
    lib = _lib.load()
    td = model.device_tris()
    pj = np.ascontiguousarray(proj, np.float32)
    roi = _lib.Roi(0, 0, 0, 0)
    out = {"workload": "configs[1] contour check: obj_06.ply, 256 refined synth hypotheses, 640x480; (a) pr_score_contours without overlap, "
                       "(b) pr_score_poses, (c) pr_render_to_host of the same poses, (d) pr_scene_edge_distance_dev",
           "tau_mm": args.tau, "jump_mm": args.jump, "radius": args.radius, "warmup_calls": args.warmup, "calls": args.calls}
    frames = np.empty((P, H, W), np.int32) if args.only in (None, "c") else None
    for name, dt in (("int32", np.int32), ("uint16", np.uint16)):
        sd = api.DeviceVector.from_host(depth.astype(dt).reshape(-1))
        ed = api.scene_edge_distance(sd, W, H, args.jump, args.radius)
        scores = np.zeros(P, api.SCORE)
        scores_b = np.zeros(P, api.SCORE)
        con = np.zeros(P, api.CONTOUR)
        cases = {
            "a": lambda: lib.pr_score_contours(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(),
                                               int(dt == np.int32), args.tau, args.jump, ed.data(), scores.ctypes.data, con.ctypes.data, None),
            "b": lambda: lib.pr_score_poses(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(),
                                            int(dt == np.int32), args.tau, scores_b.ctypes.data),
            "c": lambda: lib.pr_render_to_host(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, frames.ctypes.data),
            "d": lambda: lib.pr_scene_edge_distance_dev(sd.data(), int(dt == np.int32), W, H, args.jump, args.radius, ed.data()),
        }
        r = {k: timed(cases[k], args.warmup, args.calls) for k in ("a", "b", "c", "d") if args.only in (None, k)}
        if args.only is None:
            assert scores.tobytes() == scores_b.tobytes()
            assert np.array_equal(con["contour"].astype(np.int64), con["hit"].astype(np.int64) + con["occluded"] + con["miss"])
            r["a_minus_b_ms"] = round(r["a"]["median_ms"] - r["b"]["median_ms"], 4)
            r["a_beats_c"] = bool(r["a"]["max_ms"] < r["c"]["min_ms"])
        if args.only in (None, "a"):
            r["contour_sum"] = int(con["contour"].sum())
            r["hit_sum"] = int(con["hit"].sum())
            r["median_contour_fraction"] = round(float(np.median(api.contour_fraction(con))), 4)
        out[name] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
