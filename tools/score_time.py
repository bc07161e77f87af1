#!/usr/bin/env python
"""Wall time of one pr_score_poses call on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations),
640x480, scored against the bench's int32 scene and against a uint16 copy of it.  One JSON line: per scene dtype, ms per call (median /
min / max over --calls calls after --warmup calls) and the sum of `visible` as a sanity figure.

    python tools/score_time.py [--calls 100] [--warmup 10] [--tau 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pose_refine_amd import _lib, api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tau", type=int, default=5)
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
    lib = _lib.load()
    td = model.device_tris()
    pj = np.ascontiguousarray(proj, np.float32)
    out = {"workload": "configs[1] scoring: obj_06.ply, 256 refined synth hypotheses, 640x480, one pr_score_poses call",
           "tau_mm": args.tau, "warmup_calls": args.warmup, "calls": args.calls}
    for name, dt in (("int32", np.int32), ("uint16", np.uint16)):
        sd = api.DeviceVector.from_host(depth.astype(dt).reshape(-1))
        scores = np.zeros(len(refined), api.SCORE)
        call = lambda: lib.pr_score_poses(td.data(), td.size() // 9, refined.ctypes.data, len(refined), W, H, pj.ctypes.data,  # noqa: E731
                                          _lib.Roi(0, 0, 0, 0), sd.data(), int(dt == np.int32), args.tau, scores.ctypes.data)
        for _ in range(args.warmup):
            _lib.check(call())
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            rc = call()
            ms.append((time.perf_counter() - t0) * 1e3)
            _lib.check(rc)
        out[name] = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
                     "visible_sum": int(scores["visible"].sum()), "inlier_sum": int(scores["inlier"].sum())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
