#!/usr/bin/env python
"""What the interpenetration matrix costs on configs[1]: obj_06, the 256 synth hypotheses refined by one refine_batch (20 iterations), 640x480.
Three cases interleaved call by call after --warmup calls, ms per call as median / min / max over --calls calls (host clocks around the synchronous
calls): (a) pr_pose_penetration, (b) pr_score_overlap on the same poses against the bench's int32 scene -- the nearest existing call in shape, one
render and a P x P pass --, (c) pr_render_to_host of the same poses -- half the information (the near surface only) by the only other route.  Then the
planted frame of tests/solid_ref.py on the device: the pixels both render and the shared fraction of the smaller volume for S against each of its four
neighbours, and what pr_select_disjoint keeps.  One JSON line; --readme writes the profile's README from it and keeps the file's hand-written part,
everything from the line `## Kernel resources` on.

    python tools/penetration_time.py [--calls 100] [--warmup 10] [--slack 0] [--tau 5] [--readme FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pose_refine_amd import _lib, api, synth  # noqa: E402
from pose_accuracy import interleaved  # noqa: E402
from solid_ref import PLANTED_SHIFTS, planted  # noqa: E402


README = """# Interpenetration of detections (`pr_pose_penetration`): cost and use

Written by `tools/penetration_time.py --readme` on an MI355X; the JSON line it printed is at the end.

Workload: configs[1] -- obj_06, the 256 synth hypotheses refined by one `refine_batch` (20 iterations), 640x480; slack {slack_mm} mm; (b) against
the bench's scene frame as int32, tau {tau_mm} mm.  Host clocks around the synchronous calls, {calls} calls after {warmup_calls} warm-up calls, the
three cases interleaved call by call; ms per call as median (min .. max).

| case | ms per call |
|---|---|
| (a) `pr_pose_penetration`: span render of 256 boxes, 256 x 256 records of 24 bytes | {a} |
| (b) `pr_score_overlap`: one render, scores, bit planes, 256 x 256 counts of 4 bytes | {b} |
| (c) `pr_render_to_host`: 256 full near frames to the host (the far surface cannot be had this way at all) | {c} |

(a) / (b) = {a_over_b}, (a) / (c) = {a_over_c}.  {verdict}

## The planted frame on the device

`S = synth.scene_pose()` against its four neighbours (tests/solid_ref.py `planted()`), slack 0; next to the figures of the numpy prototype the check
was proposed with.  `pr_select_disjoint` with the rule 1/10 over the order [S, S+(8,4,0), S+(0,0,120), S+(150,40,0), S+(25,0,0)] keeps {kept}.

| pair | pixels both render | shared volume / smaller volume | prototype |
|---|---|---|---|
{planted_rows}

```
{json}
```
{kept_text}"""
KEPT_FROM = "## Kernel resources"
PROTOTYPE = {(0, 0, 120): "10 796, 0", (25, 0, 0): "13 277, 0.470", (8, 4, 0): "18 107, 0.760", (150, 40, 0): "0, 0"}


def write_readme(path, out):
    def cell(r):
        return f"{r['median_ms']} ({r['min_ms']} .. {r['max_ms']})"
    a, b, c = out["a"], out["b"], out["c"]
    if a["max_ms"] < c["min_ms"]:
        verdict = "(a) is below (c): the slowest call of (a) was faster than the fastest of (c)."
    elif a["median_ms"] < c["median_ms"]:
        verdict = "(a) is below (c) at the median, but the ranges overlap."
    else:
        verdict = "(a) is NOT below (c)."
    rows = [f"| `S`, `S + {tuple(p['shift'])}` | {p['both']} | {p['fraction']} | {PROTOTYPE[tuple(p['shift'])]} |" for p in out["planted"]]
    kept = ""
    if os.path.exists(path):
        old = open(path).read()
        if KEPT_FROM in old:
            kept = "\n" + old[old.index(KEPT_FROM):]
    text = README.format(a=cell(a), b=cell(b), c=cell(c), a_over_b=out["a_over_b"], a_over_c=out["a_over_c"], verdict=verdict, kept=out["planted_kept"],
                         planted_rows="\n".join(rows), json=json.dumps(out), kept_text=kept,
                         **{k: out[k] for k in ("slack_mm", "tau_mm", "calls", "warmup_calls")})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--slack", type=int, default=0)
    ap.add_argument("--tau", type=int, default=5)
    ap.add_argument("--readme")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls: at least 50")
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, np.ascontiguousarray(synth.K_TEST)
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
    sd = api.DeviceVector.from_host(depth.astype(np.int32).reshape(-1))
    pairs, scores, ov = np.zeros((P, P), api.PAIR_SOLID), np.zeros(P, api.SCORE), np.zeros((P, P), np.uint32)
    frames = np.zeros((P, H, W), np.int32)
    cases = {
        "a": lambda: _lib.check(lib.pr_pose_penetration(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, args.slack, pairs.ctypes.data)),
        "b": lambda: _lib.check(lib.pr_score_overlap(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, sd.data(), 1, args.tau,
                                                     scores.ctypes.data, ov.ctypes.data)),
        "c": lambda: _lib.check(lib.pr_render_to_host(td.data(), td.size() // 9, refined.ctypes.data, P, W, H, pj.ctypes.data, roi, frames.ctypes.data)),
    }
    out = {"workload": "configs[1] interpenetration: obj_06.ply, 256 refined synth hypotheses, 640x480; (a) pr_pose_penetration, (b) pr_score_overlap, "
                       "(c) pr_render_to_host",
           "library": os.path.basename(_lib.LIB_PATH), "slack_mm": args.slack, "tau_mm": args.tau, "warmup_calls": args.warmup, "calls": args.calls}
    out.update(interleaved(cases, args.calls, args.warmup))
    # the matrix is what it claims to be: symmetric, bounded by its diagonal, and its `both` of the diagonal is the render's pixel count
    assert pairs.tobytes() == np.ascontiguousarray(pairs.T).tobytes()
    diag = np.diag(pairs["sum_mm"])
    assert (pairs["sum_mm"] <= np.minimum(diag[:, None], diag[None, :])).all()
    assert np.array_equal(np.diag(pairs["both"]), (frames > 0).reshape(P, -1).sum(1))
    out["a_over_b"] = round(out["a"]["median_ms"] / out["b"]["median_ms"], 3)
    out["a_over_c"] = round(out["a"]["median_ms"] / out["c"]["median_ms"], 3)
    out["a_below_c"] = bool(out["a"]["max_ms"] < out["c"]["min_ms"])
    frac = api.penetration_fraction(pairs)
    off = ~np.eye(P, dtype=bool)
    out["refined_pairs"] = {"both_gt0": int((pairs["both"][off] > 0).sum() // 2), "inter_gt0": int((pairs["inter"][off] > 0).sum() // 2),
                            "fraction_median": round(float(np.median(frac[off])), 4), "fraction_max": round(float(frac[off].max()), 4)}
    pl = api.pose_penetration(model, planted(), W, H, proj, 0)
    pf = api.penetration_fraction(pl)
    out["planted"] = [{"shift": list(PLANTED_SHIFTS[j]), "both": int(pl["both"][0, j]), "inter": int(pl["inter"][0, j]), "fraction": round(float(pf[0, j]), 3)}
                      for j in (2, 4, 1, 3)]
    out["planted_kept"] = api.select_disjoint(np.arange(5), pl).tolist()
    print(json.dumps(out), flush=True)
    if args.readme:
        write_readme(args.readme, out)


if __name__ == "__main__":
    main()
