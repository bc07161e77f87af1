#!/usr/bin/env python
"""What the robust ICP weights (api.Robust: Huber, Tukey, Cauchy) cost and find, on the configs[1] inputs: 256 obj_06 hypotheses, 640x480,
20 iterations, device solve, synchronous refine_batch.
  time       plain refine_batch and refine_batch(robust=...) per kind (c = 5 mm), INTERLEAVED call by call in one process, on the projective, the
             grid (2 mm cells) and the kd-tree scene: host clocks around the calls after warm-up; median / min / max ms per batch and robust / plain.
             A robust refine_batch runs as a one-level stride-1 pyramid, so the plain one-level refine_pyramid is timed beside it: robust against
             THAT is what the weight costs, plain pyramid against plain refine_batch what the route costs.
  kernel     one scene and case at a time, five timed batches (option profile = 1): the correspondence launches' time per launch.
  accuracy   (--accuracy) a frame that is NOT the truth's render: the object at synth.scene_pose(), a table plane 40 mm behind its far side and an
             occluder (synth.uv_sphere_mesh) in front of about a quarter of its silhouette, composed by minimum depth from pr_render_multi's images.
             synth.hypotheses(256) refined plainly, with each kind at c = 2, 5, 10, 20 mm and with a two-level anneal (20 mm, then 5 mm; ten
             iterations each at stride 1), on the three scenes, on the cluttered and on the clean frame: ADD < 0.1 d, MSSD < 1 mm, median ADD and
             the VSD recall against the frame, as tools/pose_accuracy.py forms them.
One JSON line per step (time, then kernel; or accuracy).

    python tools/robust_time.py [--calls 20] [--warmup 3] [--accuracy]
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

W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
CRIT = (0.0, 0.0, 20)
KINDS = {"huber": api.ROBUST_HUBER, "tukey": api.ROBUST_TUKEY, "cauchy": api.ROBUST_CAUCHY}
SCALES_MM = (2.0, 5.0, 10.0, 20.0)
ANNEAL_LEVELS, ANNEAL_MM = ((1, (0.0, 0.0, 10)), (1, (0.0, 0.0, 10))), (20.0, 5.0)
GRID_CELL_MM = 2.0


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def interleaved(cases, calls, warmup):
    """Every case once per round, round after round: drift of the box hits all cases alike."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    ms = {k: [] for k in cases}
    for _ in range(calls):
        for k, fn in cases.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def diameter(v):
    v = np.asarray(v, np.float64)
    sq = (v * v).sum(1)
    best = 0.0
    for i in range(0, len(v), 1024):
        best = max(best, float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v[i:i + 1024] @ v.T)).max()))
    return float(np.sqrt(best))


def scenes_of(depth):
    nn = api.Scene_nn().init_Scene_nn_cuda(depth, K)
    return {"projective": api.Scene_projective().init_Scene_projective_cuda(depth, K), f"grid_{GRID_CELL_MM:g}mm": api.Scene_grid.from_scene_nn(nn, GRID_CELL_MM * 1e-3),
            "kdtree": nn}


def step_time(args, model, proj, depth, poses):
    crit = api.ICPConvergenceCriteria(*CRIT)
    out = {}
    for name, s in scenes_of(depth).items():
        cases = {"plain": lambda s=s: api.refine_batch(model, poses, W, H, proj, K, s, crit),
                 "plain_pyramid": lambda s=s: api.refine_pyramid(model, poses, W, H, proj, K, s, levels=((1, CRIT),))}
        for k, kind in KINDS.items():
            rb = api.Robust(kind, 0.005)
            cases[k] = lambda s=s, rb=rb: api.refine_batch(model, poses, W, H, proj, K, s, crit, robust=rb)
        r = interleaved(cases, args.calls, args.warmup)
        for k in KINDS:
            r[k]["ratio_to_plain"] = round(r[k]["median_ms"] / r["plain"]["median_ms"], 4)
            r[k]["ratio_to_plain_pyramid"] = round(r[k]["median_ms"] / r["plain_pyramid"]["median_ms"], 4)
        out[name] = r
    return {"solve": "device", "calls": args.calls, "warmup_calls": args.warmup, "c_mm": 5.0, "scenes": out}


def step_kernel(args, model, proj, depth, poses):
    """Per scene and case: the correspondence launches of five timed batches (option profile = 1: a timed batch runs as one pose group)."""
    out = {}
    for name, s in scenes_of(depth).items():
        cases = {"plain_pyramid": None}
        cases.update({k: api.Robust(kind, 0.005) for k, kind in KINDS.items()})
        r = {}
        for k, rb in cases.items():
            call = lambda: api.refine_pyramid(model, poses, W, H, proj, K, s, levels=((1, CRIT),), robust=rb)  # noqa: E731
            for _ in range(args.warmup):
                call()
            api.set_option("profile", 1)
            try:
                api.profile_reset()
                for _ in range(5):
                    call()
                p = api.profile_read()
            finally:
                api.set_option("profile", 0)
            n = max(1, p["icp_launches"])
            r[k] = {"pass_launches": int(p["icp_launches"]), "pass_ms_per_batch": round(p["icp_kernel_ms"] / 5, 4), "pass_us_per_launch": round(p["icp_kernel_ms"] * 1e3 / n, 3),
                    "points_per_batch": int(p["icp_points"] // 5)}
        for k in KINDS:
            r[k]["ratio_to_plain"] = round(r[k]["pass_us_per_launch"] / r["plain_pyramid"]["pass_us_per_launch"], 4)
        out[name] = r
    return {"solve": "device", "timed_batches": 5, "c_mm": 5.0, "note": "a kd-tree pass is four kernels inside one timed launch", "scenes": out}


def cluttered_frame(model, proj):
    """(frame depth int32 mm, fraction of the object's silhouette the occluder hides, the table's depth)."""
    gt = synth.scene_pose()
    sphere = api.Model(tris=synth.uv_sphere_mesh(64, 32))
    obj = api.render_host(model, gt[None], W, H, proj)[0].astype(np.int64)
    sil = obj > 0
    table = int(obj.max()) + 40                                    # a fronto-parallel plane 40 mm behind the object's far side
    xs = np.nonzero(sil.any(0))[0]
    best = None
    for shift in np.linspace(0.0, 160.0, 33):                      # the occluder slides in from the side, 150 mm nearer the camera than the object
        p = np.eye(4, dtype=np.float32)
        p[:3, 3] = gt[:3, 3] + np.array([-shift if xs.mean() < W / 2 else shift, 0.0, -150.0], np.float32)
        imgs = api.render_multi([model, sphere], np.array([0, 1], np.uint32), np.stack([gt, p]), W, H, proj).to_host().reshape(2, H, W).astype(np.int64)
        hidden = float(((imgs[1] > 0) & (imgs[1] < imgs[0]) & sil).sum()) / float(sil.sum())
        if best is None or abs(hidden - 0.25) < abs(best[0] - 0.25):
            best = (hidden, imgs)
    hidden, imgs = best
    big = np.iinfo(np.int64).max
    stack = np.stack([np.where(imgs[0] > 0, imgs[0], big), np.where(imgs[1] > 0, imgs[1], big), np.full((H, W), table, np.int64)])
    return stack.min(0).astype(np.int32), hidden, table


def errors(model, poses, gt, diam, frame_dev, proj):
    d = api.pose_distance(model, poses, gt, None, K)
    add, mssd = api.mean_displacement(d), api.max_displacement(d)
    taus = [t * diam for t in api.VSD_TAUS_BOP]
    ve = api.vsd_errors(api.pose_vsd(model, poses, gt, W, H, proj, frame_dev, K, api.VSD_DELTA_BOP, taus), len(taus))
    return {"add_below_0.1_diameter": int((add < 0.1 * diam).sum()), "mssd_below_1mm": int((mssd < 1.0).sum()), "add_mm_median": round(float(np.median(add)), 4),
            "recall_vsd": round(float(api.vsd_recall(ve)), 4)}


def step_accuracy(model, proj, clean, poses):
    gt, diam = synth.scene_pose(), diameter(model.vertices)
    crit = api.ICPConvergenceCriteria(*CRIT)
    clutter, hidden, table = cluttered_frame(model, proj)
    out = {"diameter_mm": round(diam, 3), "occluded_fraction_of_silhouette": round(hidden, 4), "table_depth_mm": table, "grid_cell_mm": GRID_CELL_MM,
           "anneal": {"levels": [[s, list(c)] for s, c in ANNEAL_LEVELS], "c_mm": list(ANNEAL_MM)}}
    for fname, depth in (("cluttered", clutter), ("clean", clean.astype(np.int32))):
        frame_dev = api.DeviceVector.from_host(np.ascontiguousarray(depth, np.int32).reshape(-1))
        fr = {"unrefined": errors(model, poses, gt, diam, frame_dev, proj)}
        for sname, s in scenes_of(depth).items():
            r = {}
            run = lambda **kw: errors(model, api.refined_poses(api.refine_batch(model, poses, W, H, proj, K, s, crit, **kw)[0], poses), gt, diam, frame_dev, proj)  # noqa: E731
            r["plain"] = run()
            for k, kind in KINDS.items():
                for mm in SCALES_MM:
                    r[f"{k}_{mm:g}mm"] = run(robust=api.Robust(kind, mm * 1e-3))
                rec = api.refine_pyramid(model, poses, W, H, proj, K, s, levels=ANNEAL_LEVELS, robust=[api.Robust(kind, mm * 1e-3) for mm in ANNEAL_MM])[0]
                r[f"{k}_anneal"] = errors(model, api.refined_poses(rec, poses), gt, diam, frame_dev, proj)
            fr[sname] = r
        out[fname] = fr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--accuracy", action="store_true", help="the clutter table instead of the timing table")
    args = ap.parse_args()
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    poses = synth.hypotheses(256)
    if args.accuracy:
        print(json.dumps({"accuracy": step_accuracy(model, proj, depth, poses)}), flush=True)
    else:
        print(json.dumps({"time": step_time(args, model, proj, depth, poses)}), flush=True)
        print(json.dumps({"kernel": step_kernel(args, model, proj, depth, poses)}), flush=True)


if __name__ == "__main__":
    main()
