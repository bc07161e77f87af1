#!/usr/bin/env python
"""What the normal agreement costs on configs[1], and what it says: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations),
640x480, against the bench's int32 scene and a uint16 copy of it; step 4, jump 20 mm, cos 30 degrees.  Per scene dtype, ms per call (median /
min / max over --calls calls after --warmup calls, the two cases interleaved call by call) of (a) pr_score_normals without the overlap matrix
and (b) pr_score_poses on the same inputs; `a_minus_b_ms` is the price of the normal records.  --parent-json FILE adds (b) at the parent
commit: the JSON line of `tools/contour_time.py --only b` (the same call on the same inputs) run in a checkout of that commit with the same
--calls, --warmup and --tau, so the score path can be compared across the commits.  Then normal_fraction of the hypotheses that tools/pose_accuracy.py's test accepts (ADD < 0.1 x the model diameter against
synth.scene_pose()) against those it rejects.  One JSON line; --readme writes the profile's README from it and keeps the file's hand-written
part, everything from the line `## Kernel time` on.

    python tools/normals_time.py [--calls 100] [--warmup 10] [--tau 5] [--step 4] [--jump 20] [--cos-deg 30] [--parent-json FILE] [--readme FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pose_refine_amd import _lib, api, synth  # noqa: E402
from pose_accuracy import diameter, stats  # noqa: E402


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


def group(frac):
    if len(frac) == 0:
        return {"n": 0}
    return {"n": int(len(frac)), "min": round(float(frac.min()), 4), "median": round(float(np.median(frac)), 4), "max": round(float(frac.max()), 4)}


README = """# Normal agreement (`pr_score_normals`): cost and use

Written by `tools/normals_time.py --readme` on an MI355X; the JSON line it printed is at the end.

Workload: configs[1] -- obj_06, the 256 synth hypotheses refined by one `refine_batch` (20 iterations), 640x480, the bench's scene frame as
int32 and as uint16; tau {tau_mm} mm, step {step}, jump {jump_mm} mm, cos_min = cos {cos_deg} degrees.  Host clocks around the synchronous calls,
{calls} calls after {warmup_calls} warm-up calls, the cases interleaved call by call; ms per call as median (min .. max).

| scene | (a) `pr_score_normals` | (b) `pr_score_poses` | a - b | (b) from the parent commit's build |
|---|---|---|---|---|
{rows}

`normal_box_kernel<int32_t>` uses 70 VGPRs, `normal_box_kernel<uint16_t>` 68; both use no scratch and 80 bytes of LDS (`block_totals`), as the
compiler reports them (`-Rpass-analysis=kernel-resource-usage`): 7 waves per SIMD.

## What the fraction says

`normal_fraction` of the refined hypotheses that `tools/pose_accuracy.py`'s test accepts (ADD < 0.1 x the model diameter of {diameter_mm} mm against
`synth.scene_pose()`) and of those it rejects, int32 scene:

| | n | min | median | max |
|---|---|---|---|---|
| accepted | {acc} |
| rejected | {rej} |

```
{json}
```
{kept}"""
KEPT_FROM = "## Kernel time"


def write_readme(path, out):
    def cell(r):
        return f"{r['median_ms']} ({r['min_ms']} .. {r['max_ms']})"
    rows = []
    for name in ("int32", "uint16"):
        r = out[name]
        parent = cell(out["parent"][name]["b"]) if "parent" in out else "not measured"
        rows.append(f"| {name} | {cell(r['a'])} | {cell(r['b'])} | {r['a_minus_b_ms']} | {parent} |")
    g = out["fraction"]

    def grow(d):
        return f"{d['n']} | " + (f"{d['min']} | {d['median']} | {d['max']}" if d["n"] else "- | - | -")
    kept = ""
    if os.path.exists(path):
        old = open(path).read()
        if KEPT_FROM in old:
            kept = "\n" + old[old.index(KEPT_FROM):]
    text = README.format(rows="\n".join(rows), kept=kept, acc=grow(g["accepted"]), rej=grow(g["rejected"]), json=json.dumps(out), **{
        k: out[k] for k in ("tau_mm", "step", "jump_mm", "cos_deg", "calls", "warmup_calls", "diameter_mm")})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--jump", type=int, default=20)
    ap.add_argument("--cos-deg", type=float, default=30.0)
    ap.add_argument("--parent-json")
    ap.add_argument("--readme")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls: at least 50")
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, np.ascontiguousarray(synth.K_TEST)
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    depth = api.render_host(model, gt[None], W, H, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    poses = synth.hypotheses(256)
    res, _ = api.refine_batch(model, poses, W, H, proj, K, scene, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = np.ascontiguousarray(api.refined_poses(res, poses).reshape(-1, 16))
    P = len(refined)
    lib = _lib.load()
    td = model.device_tris()
    pj = np.ascontiguousarray(proj, np.float32)
    roi = _lib.Roi(0, 0, 0, 0)
    cos_min = float(np.cos(np.deg2rad(args.cos_deg)))
    out = {"workload": "configs[1] normal agreement: obj_06.ply, 256 refined synth hypotheses, 640x480; (a) pr_score_normals without overlap, (b) pr_score_poses",
           "library": os.path.basename(_lib.LIB_PATH), "tau_mm": args.tau, "step": args.step, "jump_mm": args.jump, "cos_deg": args.cos_deg,
           "warmup_calls": args.warmup, "calls": args.calls}
    for name, dt in (("int32", np.int32), ("uint16", np.uint16)):
        sd = api.DeviceVector.from_host(depth.astype(dt).reshape(-1))
        scores, scores_b = np.zeros(P, api.SCORE), np.zeros(P, api.SCORE)
        cases = {"b": lambda: lib.pr_score_poses(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(), int(dt == np.int32),
                                                 args.tau, scores_b.ctypes.data)}
        nrm = np.zeros(P, api.NORMAL)
        cases["a"] = lambda: lib.pr_score_normals(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(), int(dt == np.int32),
                                                  args.tau, K.ctypes.data, args.step, args.jump, cos_min, scores.ctypes.data, nrm.ctypes.data, None)
        r = interleaved(cases, args.calls, args.warmup)
        assert scores.tobytes() == scores_b.tobytes()
        n64 = {f: nrm[f].astype(np.int64) for f in ("tested", "agree", "disagree", "no_render_normal", "no_scene_normal")}
        assert np.array_equal(n64["tested"], n64["agree"] + n64["disagree"])
        assert np.array_equal(scores["inlier"].astype(np.int64), n64["tested"] + n64["no_render_normal"] + n64["no_scene_normal"])
        r["a_minus_b_ms"] = round(r["a"]["median_ms"] - r["b"]["median_ms"], 4)
        r.update({f + "_sum": int(v.sum()) for f, v in n64.items()})
        if name == "int32":
            diam = diameter(model.vertices)
            add = api.mean_displacement(api.pose_distance(model, refined.reshape(-1, 4, 4), gt))
            ok = add < 0.1 * diam
            frac = api.normal_fraction(nrm)
            out["diameter_mm"] = round(diam, 3)
            out["fraction"] = {"accepted": group(frac[ok]), "rejected": group(frac[~ok])}
        out[name] = r
    if args.parent_json:
        # the same score path at the parent commit: the JSON line of `tools/contour_time.py --only b` run in a checkout of that commit (same
        # 256 refined hypotheses, frame and scenes; this library cannot stand in for it, and that one has no pr_score_normals)
        with open(args.parent_json) as f:
            parent = json.loads(f.read().strip().splitlines()[-1])
        if parent["tau_mm"] != args.tau or parent["calls"] != args.calls or parent["warmup_calls"] != args.warmup:
            sys.exit(f"{args.parent_json}: taken with other --tau, --calls or --warmup")
        out["parent"] = {name: {"b": parent[name]["b"]} for name in ("int32", "uint16")}
    print(json.dumps(out), flush=True)
    if args.readme:
        write_readme(args.readme, out)


if __name__ == "__main__":
    main()
