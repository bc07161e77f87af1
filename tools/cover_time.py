#!/usr/bin/env python
"""What the cover selection costs, against the floor and the route it replaces, on the same poses in one process:
(a) pr_score_cover (render, score, support bits, the walk on the device), (b) pr_score_poses (the floor: render and score alone),
(c) pr_score_overlap + select_hypotheses (the P x P matrix and the pairwise rule on the host).  Two frames, 640x480, obj_06:
"configs1" -- the 256 synth hypotheses refined by one refine_batch (20 iterations) against the bench's scene --, and "planted" -- the 255
hypotheses of the planted frame (tests/select_ref.py's construction, the scene from the library's own render).  Each at P = 256 (255),
1024 and 4096 hypotheses, the larger batches tiling the first.  The three cases are interleaved call by call; per case ms per call (median /
min / max over --calls calls after --warmup calls of each), the rounds the walk took, and the device memory each route holds for the call.
The order walked is rank_hypotheses of the batch's scores, the rule (1, 2), min_new = 1.  One JSON line.

    python tools/cover_time.py [--calls 50] [--warmup 5] [--tau 5] [--sizes 256,1024,4096] [--only a|b|c]      (--only: one case, for a profiler run)
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

PLANTED_SHIFTS = ((-70, 0, 60), (0, 0, 0), (150, 40, 0))


def shift(dx, dy, dz):
    m = np.zeros((4, 4), np.float32)
    m[:3, 3] = (dx, dy, dz)
    return m


def planted(model, W, H, proj):
    """Three instances of the object and 85 hypotheses around each (the exact pose first); the scene: the front-most of the three renders."""
    S = synth.scene_pose()
    inst = [S + shift(*d) for d in PLANTED_SHIFTS]
    r = api.render_host(model, np.stack(inst), W, H, proj).astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    hy = synth.hypotheses(256)
    poses = [inst[k] if j < 0 else hy[1 + 84 * k + j] + shift(*PLANTED_SHIFTS[k]) for k in range(3) for j in range(-1, 84)]
    return scene.astype(np.int32), np.stack(poses).astype(np.float32)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def measure(model, poses, scene, W, H, proj, tau, warmup, calls, only):
    lib = _lib.load()
    td = model.device_tris()
    pj = np.ascontiguousarray(proj, np.float32)
    roi = _lib.Roi(0, 0, 0, 0)
    poses = np.ascontiguousarray(poses.reshape(-1, 16), np.float32)
    P = len(poses)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    sc_a, sc_b, sc_c = np.zeros(P, api.SCORE), np.zeros(P, api.SCORE), np.zeros(P, api.SCORE)
    cov, frame = np.zeros(P, api.COVER), np.zeros(1, api.COVER_FRAME)
    sel, n_sel = np.zeros(P, np.uint32), _lib.C.c_uint32(0)
    with_matrix = P <= api.OVERLAP_MAX_POSES
    ov = np.zeros((P, P), np.uint32) if with_matrix and only in (None, "c") else None
    head = (td.data(), td.size() // 9, poses.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(), 1, tau)
    _lib.check(lib.pr_score_poses(*head, sc_b.ctypes.data))
    order = np.ascontiguousarray(api.rank_hypotheses(sc_b), np.uint32)
    picked = {}

    def a():
        _lib.check(lib.pr_score_cover(*head, order.ctypes.data, P, 1, 2, 1, 0xffffffff, sc_a.ctypes.data, cov.ctypes.data, frame.ctypes.data,
                                      sel.ctypes.data, _lib.C.byref(n_sel)))

    def b():
        _lib.check(lib.pr_score_poses(*head, sc_b.ctypes.data))

    def c():
        _lib.check(lib.pr_score_overlap(*head, sc_c.ctypes.data, ov.ctypes.data))
        picked["c"] = api.select_hypotheses(sc_c, ov, max_shared=(1, 2))

    cases = {k: f for k, f in (("a", a), ("b", b), ("c", c)) if only in (None, k) and (k != "c" or with_matrix)}
    ms = {k: [] for k in cases}
    for it in range(warmup + calls):
        for k, f in cases.items():                                 # interleaved: the three see the same machine
            t0 = time.perf_counter()
            f()                                                    # (every entry point returns with its stream drained)
            if it >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    r = {k: stats(v) for k, v in ms.items()}
    wpr = (W + 63) // 64
    r["poses"] = P
    r["planes_mb"] = round(P * H * wpr * 8 / 2**20, 2)
    r["cover_extra_mb"] = round((H * wpr * 8 + 4 * (8 + 5 * P + 2 * P)) / 2**20, 3)
    r["matrix_mb_device_and_pinned"] = round(2 * 4 * P * P / 2**20, 2) if with_matrix else None
    if "a" in cases:
        assert sc_a.tobytes() == sc_b.tobytes()
        r["selected"] = int(n_sel.value)
        r["rounds"] = int(min(n_sel.value + 1, P + 1))
        r["claimed"] = int(frame["claimed"][0])
    if "c" in cases:
        r["selected_by_matrix_route"] = int(len(picked["c"]))
    if "a" in cases and "c" in cases:
        r["a_over_c"] = round(r["a"]["median_ms"] / r["c"]["median_ms"], 3)
    if "a" in cases and "b" in cases:
        r["a_minus_b_ms"] = round(r["a"]["median_ms"] - r["b"]["median_ms"], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--only", choices=["a", "b", "c"])
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    sizes = [int(v) for v in args.sizes.split(",")]
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    hy = synth.hypotheses(256)
    res, _ = api.refine_batch(model, hy, W, H, proj, K, scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    frames = {"configs1": (np.ascontiguousarray(depth, np.int32), api.refined_poses(res, hy)), "planted": planted(model, W, H, proj)}
    out = {"workload": "obj_06.ply, 640x480, int32 scene; (a) pr_score_cover, (b) pr_score_poses, (c) pr_score_overlap + select_hypotheses; rule (1, 2), "
                       "min_new 1, order = rank_hypotheses", "tau_mm": args.tau, "warmup_calls": args.warmup, "calls": args.calls}
    for name, (sc, poses) in frames.items():
        out[name] = []
        for n in sizes:
            tiled = poses if n <= 256 else np.concatenate([poses] * ((n + len(poses) - 1) // len(poses)))[:n]      # (the planted frame: 255)
            out[name].append(measure(model, tiled, sc, W, H, proj, args.tau, args.warmup, args.calls, args.only))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
