#!/usr/bin/env python
"""What contour alignment costs and does on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations), 640x480,
the bench's scene frame (int32).  One JSON line.

  time      ms per call (median / min / max over --calls calls after --warmup, the cases interleaved call by call) of (a) pr_contour_information,
            (b) pr_score_contours and (c) pr_score_poses on the same poses, (d) pr_scene_edge_nearest_dev and (e) pr_scene_edge_distance_dev,
            (f) pr_pose_information without the decomposition, (g) one api.refine_contours iteration (f + a + the host's combine, Jacobi and step).
            --parent-json FILE adds (b) at the parent commit: the JSON line of `tools/contour_time.py --only a --radius R` run against that
            commit's library (PR_LIB_PATH) with the same --calls, --warmup, --tau and --jump.
  accuracy  tools/pose_accuracy.py's ADD / MSSD counts of the 256 refined hypotheses before and after api.refine_contours, how many of the
            hypotheses that miss ADD < 0.1 d come back and how many of those that meet it get worse or are lost.
  wall      obj_06 at the model pose against a flat wall (tools/info_time.py's example: surface rank 3; a flat wall has no depth edge), and a plate
            50 mm in front of a wall seen from a pose off in the plane: the rank of the surface record and of the combined one.
  --kernels the timed device calls alone, a few times each, for a kernel trace (the per-kernel split).
  --readme  writes the profile's README from the line and keeps the file's hand-written part, everything from the line `## Kernel time` on.

    python tools/contour_fit_time.py [--calls 60] [--warmup 10] [--tau 5] [--jump 10] [--radius 8] [--iterations 4] [--weight 1] [--min-ratio 1e-6]
                                     [--min-used 32] [--parent-json FILE] [--kernels] [--readme FILE]
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
from pose_accuracy import diameter, interleaved  # noqa: E402

W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST

README = """# Contour alignment (`pr_contour_information`, `api.refine_contours`): cost and effect

Written by `tools/contour_fit_time.py --readme` on an MI355X; the JSON line it printed is at the end.

Workload: configs[1] -- obj_06, the 256 synth hypotheses refined by one `refine_batch` (20 iterations), 640x480, the bench's scene frame
(int32); tau {tau_mm} mm, jump {jump_mm} mm, nearest-edge radius {radius} px.  Host clocks around the synchronous calls, {calls} calls after
{warmup_calls} warm-up calls, the cases interleaved call by call; ms per call as median (min .. max).

| call | ms |
|---|---|
{rows}

`pr_contour_information` against `pr_score_contours` on the same poses: {a_minus_b} ms more per call for the float64 normal equations
({used_sum} used contour pixels, two rows each).{parent}

## Accuracy: `refine_contours` after `refine_batch`

{iterations} iterations, weight {weight}, min_ratio {min_ratio}, min_used {min_used}; ADD / MSSD against `synth.scene_pose()` over the model's
vertices (`tools/pose_accuracy.py`'s counts; d = {diameter} mm).

| | ADD < 0.1 d | MSSD < 1 mm | median ADD mm |
|---|---|---|---|
| after `refine_batch` | {b_add} | {b_mssd} | {b_med} |
| after `refine_contours` | {a_add} | {a_mssd} | {a_med} |

Of the {n_lost} hypotheses that miss ADD < 0.1 d after `refine_batch`, {came_back} meet it after `refine_contours`.  Of the {n_good} that meet it,
{lost_good} miss it afterwards and {worse} have an ADD more than 0.1 mm larger (largest increase {worst_increase} mm).

## Rank on a wall

| scene | surface rank | combined rank | used contour pixels |
|---|---|---|---|
{wall_rows}

"""


def r4(x):
    return round(float(x), 4)


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f} .. {s['max_ms']:.3f})"


def add_mssd(model, poses, gt):
    d = api.pose_distance(model, poses, gt, None, K)
    return api.mean_displacement(d), api.max_displacement(d)


def rank_pair(tris, pose, w, h, proj, k, frame, cm, rho, args, **scene_kw):
    scene = api.Scene_projective().init_Scene_projective_cuda(frame, k, width=w, height=h, **scene_kw)
    nd = api.scene_edge_nearest(frame, w, h, args.jump, args.radius)
    surf, eig, _ = api.pose_information(tris, pose[None], w, h, proj, k, scene, center=cm, radius=rho)
    _, fit, con = api.contour_information(tris, pose[None], w, h, proj, k, frame, args.tau, args.jump, nd, center=cm, radius=rho, want_scores=False)
    both = api.combine_information(surf, con, 1.0, args.weight)
    return {"surface_rank": int(api.observable_rank(eig, args.min_ratio)[0]), "combined_rank": int(api.observable_rank(api.information_eig(both), args.min_ratio)[0]),
            "used": int(fit[0]["used"]), "surface_lambda_over_lambda5": [float(x) for x in eig[0]["lambda"] / eig[0]["lambda"][5]]}


def wall_case(model, proj, args):
    """obj_06 at the model pose against a flat wall at its median depth (tools/info_time.py's example), and a 200 x 140 mm plate 50 mm in front of a
    wall, 160 x 120 at f = 200, seen from a pose 30 mm and 0.05 rad off in the plane (the tests' case)."""
    pose = np.asarray(synth.test_cpp_poses()[0], np.float32).reshape(4, 4)
    render = api.render_host(model, pose[None], W, H, proj)[0]
    flat = np.full((H, W), int(np.median(render[render > 0])), np.int32)
    out = {"obj_06 on a flat wall": rank_pair(model, pose, W, H, proj, K, flat, None, None, args)}
    a, b, c, d = (-100.0, -70.0, 0.0), (100.0, -70.0, 0.0), (100.0, 70.0, 0.0), (-100.0, 70.0, 0.0)
    plate = np.array([[a, b, c], [a, c, d], [a, c, b], [a, d, c]], np.float32)
    kp = np.array([200.0, 0.0, 80.0, 0.0, 200.0, 60.0, 0.0, 0.0, 1.0], np.float32)
    pp = api.compute_proj(kp, 160, 120)
    true, start = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    true[2, 3] = start[2, 3] = 1000.0
    start[:2, :2] = [[np.cos(0.05), -np.sin(0.05)], [np.sin(0.05), np.cos(0.05)]]
    start[:2, 3] = [24.0, 18.0]
    seen = api.render_host(plate, true[None], 160, 120, pp)[0]
    frame = np.where(seen > 0, seen, 1050).astype(np.int32)
    out["a plate 50 mm in front of a wall"] = rank_pair(plate, start, 160, 120, pp, kp, frame, np.zeros(3, np.float32), 0.1, args, max_dist_diff=0.01)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--jump", type=int, default=10)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--min-ratio", type=float, default=1e-6)
    ap.add_argument("--min-used", type=int, default=32)
    ap.add_argument("--parent-json")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--readme")
    args = ap.parse_args()
    api.init(0)
    api.set_option("solve", api.SOLVE_DEVICE)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    depth = np.ascontiguousarray(api.render_host(model, gt[None], W, H, proj)[0], np.int32)
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    poses = synth.hypotheses(256)
    res, _ = api.refine_batch(model, poses, W, H, proj, K, scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = np.ascontiguousarray(api.refined_poses(res, poses).reshape(-1, 4, 4))
    sd = api.DeviceVector.from_host(depth.reshape(-1))
    nd = api.scene_edge_nearest(sd, W, H, args.jump, args.radius)
    ed = api.scene_edge_distance(sd, W, H, args.jump, args.radius)
    cases = {
        "a pr_contour_information": lambda: api.contour_information(model, refined, W, H, proj, K, sd, args.tau, args.jump, nd),
        "b pr_score_contours": lambda: api.score_contours(model, refined, W, H, proj, sd, args.tau, args.jump, ed),
        "c pr_score_poses": lambda: api.score_poses(model, refined, W, H, proj, sd, args.tau),
        "d pr_scene_edge_nearest_dev": lambda: api.scene_edge_nearest(sd, W, H, args.jump, args.radius).free(),
        "e pr_scene_edge_distance_dev": lambda: api.scene_edge_distance(sd, W, H, args.jump, args.radius).free(),
        "f pr_pose_information, no eig": lambda: api.pose_information(model, refined, W, H, proj, K, scene, want_eig=False),
        "g refine_contours, 1 iteration": lambda: api.refine_contours(model, refined, W, H, proj, K, scene, sd, nd, args.tau, args.jump, iterations=1,
                                                                    weight=args.weight, min_ratio=args.min_ratio, min_used=args.min_used),
    }
    if args.kernels:
        for k, fn in cases.items():
            if k[0] in "abdf":
                for _ in range(5):
                    fn()
        return
    out = {"workload": "configs[1] contour alignment: obj_06.ply, 256 refined synth hypotheses, 640x480, int32 scene", "tau_mm": args.tau, "jump_mm": args.jump,
           "radius": args.radius, "calls": args.calls, "warmup_calls": args.warmup, "iterations": args.iterations, "weight": args.weight,
           "min_ratio": args.min_ratio, "min_used": args.min_used}
    out["time"] = interleaved(cases, args.calls, args.warmup)
    _, fit, _ = cases["a pr_contour_information"]()
    out["used_sum"], out["contour_sum"] = int(fit["used"].sum()), int(fit["contour"].sum())
    out["a_minus_b_ms"] = r4(out["time"]["a pr_contour_information"]["median_ms"] - out["time"]["b pr_score_contours"]["median_ms"])
    if args.parent_json:
        parent = json.loads(open(args.parent_json).read().strip().splitlines()[-1])
        out["parent_pr_score_contours"] = parent["int32"]["a"]
    # accuracy
    diam = diameter(model.vertices)
    after, hist = api.refine_contours(model, refined, W, H, proj, K, scene, sd, nd, args.tau, args.jump, iterations=args.iterations, weight=args.weight,
                                      min_ratio=args.min_ratio, min_used=args.min_used)
    add0, mssd0 = add_mssd(model, refined, gt)
    add1, mssd1 = add_mssd(model, after, gt)
    good0, good1 = add0 < 0.1 * diam, add1 < 0.1 * diam
    out["accuracy"] = {"diameter_mm": round(diam, 3),
                       "before": {"add_below_0.1_diameter": int(good0.sum()), "mssd_below_1mm": int((mssd0 < 1.0).sum()), "add_median_mm": r4(np.median(add0))},
                       "after": {"add_below_0.1_diameter": int(good1.sum()), "mssd_below_1mm": int((mssd1 < 1.0).sum()), "add_median_mm": r4(np.median(add1))},
                       "lost_before": int((~good0).sum()), "lost_that_come_back": int((~good0 & good1).sum()), "good_before": int(good0.sum()),
                       "good_that_are_lost": int((good0 & ~good1).sum()), "good_with_add_worse_by_0.1mm": int((good0 & (add1 > add0 + 0.1)).sum()),
                       "largest_add_increase_among_good_mm": r4((add1 - add0)[good0].max()) if good0.any() else 0.0,
                       "rank_first_iteration_histogram": np.bincount(hist["rank"][0], minlength=7).tolist(),
                       "stepped_every_iteration": int((hist["used"] >= args.min_used).all(0).sum()),
                       "rms_px_median_first_last": [r4(np.nanmedian(hist["rms_px"][0])), r4(np.nanmedian(hist["rms_px"][-1]))]}
    out["wall"] = wall_case(model, proj, args)
    print(json.dumps(out), flush=True)
    if args.readme:
        keep = ""
        if os.path.exists(args.readme):
            text = open(args.readme).read()
            at = text.find("## Kernel time")
            keep = text[at:] if at >= 0 else ""
        acc, par = out["accuracy"], ""
        if "parent_pr_score_contours" in out:
            par = f"  `pr_score_contours` built from the parent commit, same inputs: {fmt(out['parent_pr_score_contours'])} ms."
        text = README.format(rows="\n".join(f"| ({k[0]}) `{k[2:]}` | {fmt(v)} |" for k, v in out["time"].items()), a_minus_b=out["a_minus_b_ms"],
                             used_sum=out["used_sum"], parent=par, diameter=acc["diameter_mm"], b_add=acc["before"]["add_below_0.1_diameter"],
                             b_mssd=acc["before"]["mssd_below_1mm"], b_med=acc["before"]["add_median_mm"], a_add=acc["after"]["add_below_0.1_diameter"],
                             a_mssd=acc["after"]["mssd_below_1mm"], a_med=acc["after"]["add_median_mm"], n_lost=acc["lost_before"],
                             came_back=acc["lost_that_come_back"], n_good=acc["good_before"], lost_good=acc["good_that_are_lost"],
                             worse=acc["good_with_add_worse_by_0.1mm"], worst_increase=acc["largest_add_increase_among_good_mm"],
                             wall_rows="\n".join(f"| {k} | {v['surface_rank']} | {v['combined_rank']} | {v['used']} |" for k, v in out["wall"].items()),
                             **{k: out[k] for k in ("tau_mm", "jump_mm", "radius", "calls", "warmup_calls", "iterations", "weight", "min_ratio", "min_used")})
        with open(args.readme, "w") as f:
            f.write(text + (keep or "## Kernel time\n\n(to be written by hand from a kernel trace of `--kernels`)\n"))


if __name__ == "__main__":
    main()
