#!/usr/bin/env python
"""What the visible surface discrepancy costs on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations),
640x480, against the bench's int32 scene and a uint16 copy of it.  Per scene dtype, ms per call (median / min / max over --calls rounds after
--warmup rounds, the three cases interleaved call by call) of (a) pr_pose_vsd of the 256 refined hypotheses against the one true pose with
BOP's delta and ten taus, with K; (b) pr_score_poses on the same 256; (c) pr_render_to_host of the 257 poses -- the only route to the same
counts without (a), the host's classification of the 257 frames not included.  One JSON line; `a_minus_b_ms` is what the second box per pixel
and the one extra render cost over a scoring call, `a_beats_c` says whether max(a) < min(c).

    python tools/vsd_time.py [--calls 100] [--warmup 10] [--only a|b|c]      (--only: one case, for a profiler run)
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

DIAMETER = 154.546                       # obj_06, mm (tools/pose_accuracy.py computes it from the vertices)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def interleaved(cases, calls, warmup):
    """Every case once per round, round after round: drift of the box hits all cases alike."""
    for _ in range(warmup):
        for fn in cases.values():
            _lib.check(fn())
    ms = {k: [] for k in cases}
    for _ in range(calls):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            rc = fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            _lib.check(rc)
    return {k: stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["a", "b", "c"])
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls: at least 50")
    api.init(0)
    W, H = synth.WIDTH, synth.HEIGHT
    K = np.ascontiguousarray(synth.K_TEST, np.float32)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = np.ascontiguousarray(synth.scene_pose().reshape(1, 16), np.float32)
    depth = api.render_host(model, gt, W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    poses = synth.hypotheses(256)
    res, _ = api.refine_batch(model, poses, W, H, proj, K, scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = np.ascontiguousarray(api.refined_poses(res, poses).reshape(-1, 16))
    all257 = np.ascontiguousarray(np.concatenate([refined, gt]))
    P = len(refined)
    taus = np.array([t * DIAMETER for t in api.VSD_TAUS_BOP], np.float32)
    lib = _lib.load()
    td = model.device_tris()
    pj = np.ascontiguousarray(proj, np.float32)
    roi = _lib.Roi(0, 0, 0, 0)
    out = {"workload": "configs[1] VSD: obj_06.ply, 256 refined synth hypotheses against the scene pose, 640x480; (a) pr_pose_vsd (K, delta 15 mm, ten taus), "
                       "(b) pr_score_poses of the 256, (c) pr_render_to_host of the 257 poses", "warmup_calls": args.warmup, "calls": args.calls}
    frames = np.empty((P + 1, H, W), np.int32) if args.only in (None, "c") else None
    for name, dt in (("int32", np.int32), ("uint16", np.uint16)):
        sd = api.DeviceVector.from_host(depth.astype(dt).reshape(-1))
        rec = np.zeros(P, api.VSD)
        scores = np.zeros(P, api.SCORE)
        cases = {
            "a": lambda: lib.pr_pose_vsd(td.data(), td.size() // 9, refined.ctypes.data, P, gt.ctypes.data, 1, W, H, pj.ctypes.data, sd.data(),
                                         int(dt == np.int32), K.ctypes.data, api.VSD_DELTA_BOP, taus.ctypes.data, len(taus), rec.ctypes.data),
            "b": lambda: lib.pr_score_poses(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(),
                                            int(dt == np.int32), 5, scores.ctypes.data),
            "c": lambda: lib.pr_render_to_host(td.data(), td.size() // 9, all257.ctypes.data, P + 1, W, H, pj.ctypes.data, roi, frames.ctypes.data),
        }
        r = interleaved({k: cases[k] for k in ("a", "b", "c") if args.only in (None, k)}, args.calls, args.warmup)
        if args.only is None:
            r["a_minus_b_ms"] = round(r["a"]["median_ms"] - r["b"]["median_ms"], 4)
            r["a_beats_c"] = bool(r["a"]["max_ms"] < r["c"]["min_ms"])
        if args.only in (None, "a"):
            e = api.vsd_errors(rec, len(taus))
            r["uni_sum"], r["inter_sum"] = int(rec["uni"].sum()), int(rec["inter"].sum())
            r["vsd_recall"] = round(api.vsd_recall(e), 4)
        out[name] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
