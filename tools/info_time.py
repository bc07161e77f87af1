#!/usr/bin/env python
"""What pose observability (api.pose_information: pr_pose_info / pr_pose_eig) costs and what it says, on the configs[1] inputs: obj_06, the 256
synth hypotheses refined by one refine_batch (20 iterations, device solve), 640x480, the bench's scene frame.
  time      pose_information of the 256 refined hypotheses on the projective, the grid (2 mm cells) and the kd-tree scene, with and without the
            eigen-decomposition and with a Tukey weight, INTERLEAVED call by call with score_poses on the same poses (the same render, no pass) and
            with one robust refine_batch of max_iteration 0 (the same render and clouds, one score-only pass): host clocks around the synchronous
            calls after warm-up; median / min / max ms.
  shows     lambda[0] / sum_w and the observable rank over a sweep of min_ratio, separately for the hypotheses that end with ADD < 0.1 d and for the
            others (tools/pose_accuracy.py's setting), on the projective scene.
  demo      the covariance of the best hypothesis in degrees and millimetres, with the residual variance and with a 1 mm sensor sigma; and the
            weakest twist of obj_06 laid on a flat wall (the normals example: the model pose against a fronto-parallel plane).
  --kernels only the calls of `time`, five rounds, for a kernel trace from outside (one line per kernel in the profiler's statistics).
One JSON line per step.

    python tools/info_time.py [--calls 20] [--warmup 3] [--kernels]
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
GRID_CELL_MM = 2.0
RATIOS = (1e-12, 1e-9, 1e-6, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2, 3e-2, 1e-1)


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


def cases_of(model, proj, depth, scene, refined):
    frame = api.DeviceVector.from_host(np.ascontiguousarray(depth, np.int32).reshape(-1))
    tukey = api.Robust(api.ROBUST_TUKEY, 0.005)
    one_pass = api.ICPConvergenceCriteria(0.0, 0.0, 0)
    return {"score_poses": lambda: api.score_poses(model, refined, W, H, proj, frame, 5),
            "robust_one_pass": lambda: api.refine_batch(model, refined, W, H, proj, K, scene, one_pass, robust=tukey),
            "information": lambda: api.pose_information(model, refined, W, H, proj, K, scene),
            "information_no_eig": lambda: api.pose_information(model, refined, W, H, proj, K, scene, want_eig=False),
            "information_tukey": lambda: api.pose_information(model, refined, W, H, proj, K, scene, robust=tukey)}


def quantiles(v):
    v = np.asarray(v, np.float64)
    v = v[np.isfinite(v)]                                            # (a hypothesis without a correspondence has no ratio)
    return {"n": int(len(v))} if len(v) == 0 else {"n": int(len(v)), "min": float(v.min()), "q10": float(np.quantile(v, 0.1)), "median": float(np.median(v)),
                                                    "q90": float(np.quantile(v, 0.9)), "max": float(v.max())}


def step_shows(model, proj, scene, refined, diam):
    gt = synth.scene_pose()
    add = api.mean_displacement(api.pose_distance(model, refined, gt, None, K))
    ok = add < 0.1 * diam
    info, eig, sizes = api.pose_information(model, refined, W, H, proj, K, scene)
    lam = eig["lambda"]
    out = {"add_below_0.1_diameter": int(ok.sum()), "others": int((~ok).sum()), "rho_m": float(info["rho"][0]), "sweeps": quantiles(eig["sweeps"])}
    for name, sel in (("good", ok), ("others", ~ok)):
        with np.errstate(divide="ignore", invalid="ignore"):
            g = {"lambda0_over_sum_w": quantiles(lam[sel, 0] / info["sum_w"][sel]), "lambda0_over_lambda5": quantiles(lam[sel, 0] / lam[sel, 5]),
                 "n_valid_over_n_points": quantiles(info["n_valid"][sel] / np.maximum(info["n_points"][sel], 1))}
        g["rank_by_min_ratio"] = {f"{r:g}": np.bincount(api.observable_rank(eig[sel], r), minlength=7).tolist() for r in RATIOS}
        out[name] = g
    return out, info, eig, add


def cov_report(info, eig, min_ratio, sigma):
    cov, rank, s2 = api.pose_covariance(info, eig, min_ratio, sigma=sigma)
    sd = np.sqrt(np.diag(cov))
    return {"rank": rank, "sigma_mm": round(float(np.sqrt(s2)) * 1e3, 5), "rotation_sd_deg": [round(float(np.degrees(x)), 5) for x in sd[:3]],
            "translation_sd_mm": [round(float(x) * 1e3, 5) for x in sd[3:]]}


def step_demo(model, proj, info, eig, add, min_ratio):
    best = int(np.argmin(add))
    out = {"hypothesis": best, "add_mm": round(float(add[best]), 4), "n_valid": int(info[best]["n_valid"]), "min_ratio": min_ratio,
           "lambda_over_sum_w": [float(x) for x in eig[best]["lambda"] / info[best]["sum_w"]],
           "residual_variance": cov_report(info[best], eig[best], min_ratio, None), "sensor_1mm": cov_report(info[best], eig[best], min_ratio, 0.001)}
    # the normals example: obj_06 at the model pose (synth.test_cpp_poses()[0]) against a flat wall, here at the render's median depth
    pose = np.asarray(synth.test_cpp_poses()[0], np.float32).reshape(4, 4)
    render = api.render_host(model, pose[None], W, H, proj)[0]
    wall = np.full((H, W), int(np.median(render[render > 0])), np.int32)
    scene = api.Scene_projective().init_Scene_projective_cuda(wall, K)
    wi, we, _ = api.pose_information(model, pose[None], W, H, proj, K, scene)
    w, t = api.weakest_twist(wi[0], we[0], 0)
    out["on_a_flat_wall"] = {"wall_depth_mm": int(wall[0, 0]), "n_valid": int(wi[0]["n_valid"]), "lambda_over_lambda5": [float(x) for x in we[0]["lambda"] / we[0]["lambda"][5]],
                             "rank_at_min_ratio": int(api.observable_rank(we, min_ratio)[0]), "weakest_twist_omega_rad": [round(float(x), 6) for x in w],
                             "weakest_twist_t_m": [round(float(x), 6) for x in t],
                             "second_and_third": [[round(float(x), 4) for x in we[0]["V"][:, k]] for k in (1, 2)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="five rounds of the timed calls and nothing else (for a kernel trace)")
    ap.add_argument("--min-ratio", type=float, default=1e-4, help="the rank cut of the demonstration")
    args = ap.parse_args()
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    depth = api.render_host(model, synth.scene_pose()[None], W, H, proj)[0]
    scenes = scenes_of(depth)
    res, _ = api.refine_batch(model, synth.hypotheses(256), W, H, proj, K, scenes["projective"], api.ICPConvergenceCriteria(*CRIT))
    refined = np.ascontiguousarray(api.refined_poses(res, synth.hypotheses(256)).reshape(-1, 16))
    if args.kernels:
        for name, s in scenes.items():
            interleaved(cases_of(model, proj, depth, s, refined), 5, 1)
        print(json.dumps({"kernels": "five rounds per scene done"}), flush=True)
        return
    out = {name: interleaved(cases_of(model, proj, depth, s, refined), args.calls, args.warmup) for name, s in scenes.items()}
    print(json.dumps({"time": {"calls": args.calls, "warmup_calls": args.warmup, "hypotheses": 256, "scenes": out}}), flush=True)
    shows, info, eig, add = step_shows(model, proj, scenes["projective"], refined, diameter(model.vertices))
    print(json.dumps({"shows": shows}), flush=True)
    print(json.dumps({"demo": step_demo(model, proj, info, eig, add, args.min_ratio)}), flush=True)


if __name__ == "__main__":
    main()
