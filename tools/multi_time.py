#!/usr/bin/env python
"""What a mixed batch costs against the calls it replaces, on the configs[1] scene at 640x480 (host clocks around synchronous calls, after
warm-up).  Refinement (20 iterations):
  (a) one refine_batch of 256 obj_06 hypotheses;
  (b) eight refine_batch calls of 32 hypotheses each, one per mesh: obj_06, five rigidly re-posed / scaled copies of it, a second scaled
      copy and a UV sphere (synth.uv_sphere_mesh, 40 x 20 quads), each with seeded poses around the scene pose;
  (c) one refine_batch_multi of the same 256;
  (d) one refine_batch_multi of (a)'s 256 hypotheses with a one-mesh table (the mixed path against (a) on the same work).
The same for scoring: score_poses of (a), eight score_poses calls (b), one score_poses_multi (c).  One JSON line: median / min / max ms
per case over --calls repetitions.

    python tools/multi_time.py [--calls 30] [--warmup 5] [--solve device|host] [--only c]

--only a|b|c|d runs just that refinement case (a profiler run of one case).
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


def rigid(tris, angle, t, scale=1.0):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32) * np.float32(scale)
    return np.ascontiguousarray((tris.reshape(-1, 3) @ R.T + np.asarray(t, np.float32)).astype(np.float32).reshape(-1, 3, 3))


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


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
    ap.add_argument("--solve", choices=["device", "host"], default="device")
    ap.add_argument("--only", choices=["a", "b", "c", "d"], default=None)
    args = ap.parse_args()
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE if args.solve == "device" else api.SOLVE_HOST)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    obj = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(obj, synth.scene_pose()[None], W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    t = obj.tris
    host = [t, rigid(t, 0.2, (3, -2, 1)), rigid(t, -0.3, (-4, 2, 0)), rigid(t, 0.0, (0, 0, 0), 0.9), rigid(t, 0.5, (2, 2, -2), 1.1),
            rigid(t, -0.6, (0, -3, 3), 0.8), rigid(t, 1.0, (1, 0, 0), 1.05), synth.uv_sphere_mesh(40, 20)]
    meshes = [obj] + [api.Model(tris=m) for m in host[1:]]
    poses256 = synth.hypotheses(256)                              # (a): 256 obj_06 hypotheses
    per = [synth.hypotheses(32, seed=100 + m) for m in range(8)]  # (b) / (c): 32 seeded hypotheses around the scene pose per mesh
    mixed = np.concatenate(per)
    idx = np.repeat(np.arange(8), 32)

    cases = {
        "a": lambda: api.refine_batch(obj, poses256, W, H, proj, K, scene, crit),
        "b": lambda: [api.refine_batch(meshes[m], per[m], W, H, proj, K, scene, crit) for m in range(8)],
        "c": lambda: api.refine_batch_multi(meshes, idx, mixed, W, H, proj, K, scene, crit),
        "d": lambda: api.refine_batch_multi([obj], np.zeros(256, np.int64), poses256, W, H, proj, K, scene, crit),
    }
    out = {"workload": "configs[1] scene, 640x480: (a) one 256-hypothesis obj_06 call, (b) 8 meshes x 32 hypotheses as 8 calls, (c) the same as one multi call",
           "solve": args.solve, "icp_iterations": 20, "calls": args.calls, "warmup_calls": args.warmup}
    if args.only:
        out["refine_" + args.only] = timed(cases[args.only], args.calls, args.warmup)
        print(json.dumps(out), flush=True)
        return
    for k in "abcd":
        out["refine_" + k] = timed(cases[k], args.calls, args.warmup)
    sd = api.DeviceVector.from_host(depth.reshape(-1))
    score = {
        "a": lambda: api.score_poses(obj, poses256, W, H, proj, sd, 5),
        "b": lambda: [api.score_poses(meshes[m], per[m], W, H, proj, sd, 5) for m in range(8)],
        "c": lambda: api.score_poses_multi(meshes, idx, mixed, W, H, proj, sd, 5),
        "d": lambda: api.score_poses_multi([obj], np.zeros(256, np.int64), poses256, W, H, proj, sd, 5),
    }
    for k in "abcd":
        out["score_" + k] = timed(score[k], args.calls, args.warmup)
    # the multi call gives what the eight calls give
    got = api.refine_batch_multi(meshes, idx, mixed, W, H, proj, K, scene, crit)
    want = [api.refine_batch(meshes[m], per[m], W, H, proj, K, scene, crit) for m in range(8)]
    out["refine_c_equals_b"] = bool(got[0].tobytes() == np.concatenate([w[0] for w in want]).tobytes()
                                    and np.array_equal(got[1], np.concatenate([w[1] for w in want])))
    out["cloud_points_c"] = int(got[1].sum())
    out["cloud_points_a"] = int(api.refine_batch(obj, poses256, W, H, proj, K, scene, crit)[1].sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
