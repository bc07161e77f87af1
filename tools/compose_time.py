#!/usr/bin/env python
"""What the composition costs on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations), 640x480,
against the bench's int32 scene and a uint16 copy of it.  Per scene dtype, ms per call (median / min / max over --calls calls after
--warmup calls) of (a) pr_compose_detections of all 256 -- every hypothesis on the one object: the heavy case of the tile kernel --,
(b) pr_score_poses on the same inputs, (c) pr_render_to_host of the same poses -- the cheapest route to the same information without (a),
the host's per-pixel minimum over the frames not included -- and (a2) pr_compose_detections of select_hypotheses' detections only: the
intended, light case.  One JSON line; `a_minus_b_ms` is the price of the composition, `a_beats_c` says whether max(a) < min(c).

    python tools/compose_time.py [--calls 100] [--warmup 10] [--tau 5] [--only a|b|c|a2]      (--only: one case, for a profiler run)
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


def timed(call, warmup, calls):
    for _ in range(warmup):
        _lib.check(call())
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        rc = call()
        ms.append((time.perf_counter() - t0) * 1e3)
        _lib.check(rc)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b", "c", "a2"])
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
    out = {"workload": "configs[1] composition: obj_06.ply, 256 refined synth hypotheses, 640x480; (a) pr_compose_detections, (b) pr_score_poses, "
                       "(c) pr_render_to_host of the same poses, (a2) pr_compose_detections of the selected detections",
           "tau_mm": args.tau, "warmup_calls": args.warmup, "calls": args.calls}
    frames = np.empty((P, H, W), np.int32) if args.only in (None, "c") else None
    labels, front = api.DeviceVector(W * H, np.uint16), api.DeviceVector(W * H, np.int32)
    for name, dt in (("int32", np.int32), ("uint16", np.uint16)):
        sd = api.DeviceVector.from_host(depth.astype(dt).reshape(-1))
        sc, ov = api.score_overlap(model, refined, W, H, proj, sd, args.tau)
        picked = np.ascontiguousarray(refined[api.select_hypotheses(sc, ov)])
        S = len(picked)
        scores, vis, frame = np.zeros(P, api.SCORE), np.zeros(P, api.VISIBLE), np.zeros(1, api.FRAME)
        scores_b = np.zeros(P, api.SCORE)
        scores2, vis2, frame2 = np.zeros(S, api.SCORE), np.zeros(S, api.VISIBLE), np.zeros(1, api.FRAME)

        def compose(p, n, s, v, f):
            return lib.pr_compose_detections(td.data(), td.size() // 9, p.ctypes.data, n, W, H, pj.ctypes.data, roi, sd.data(), int(dt == np.int32),
                                             args.tau, labels.data(), front.data(), s.ctypes.data, v.ctypes.data, f.ctypes.data)

        cases = {
            "a": lambda: compose(refined, P, scores, vis, frame),
            "b": lambda: lib.pr_score_poses(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(),
                                            int(dt == np.int32), args.tau, scores_b.ctypes.data),
            "c": lambda: lib.pr_render_to_host(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, frames.ctypes.data),
            "a2": lambda: compose(picked, S, scores2, vis2, frame2),
        }
        r = {k: timed(cases[k], args.warmup, args.calls) for k in ("a", "b", "c", "a2") if args.only in (None, k)}
        if args.only is None:
            assert scores.tobytes() == scores_b.tobytes() and int(vis["owned"].sum()) == int(frame["covered"][0])
            r["a_minus_b_ms"] = round(r["a"]["median_ms"] - r["b"]["median_ms"], 4)
            r["a_beats_c"] = bool(r["a"]["max_ms"] < r["c"]["min_ms"])
        if args.only in (None, "a"):
            r["covered"], r["explained"], r["owners"] = int(frame["covered"][0]), int(frame["explained"][0]), int(np.count_nonzero(vis["owned"]))
        if args.only in (None, "a2"):
            r["detections"], r["a2_covered"] = S, int(frame2["covered"][0])
        out[name] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
