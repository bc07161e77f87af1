#!/usr/bin/env python3
"""Point-pair-feature voting for several models in one frame: one pr_ppf_vote_multi call against one pr_ppf_vote call per model.

The flagship frame of tools/ppf_time.py (obj_06 at synth.scene_pose(), 640x480, the library's own render, stride 4, ref_stride 5) and a table of
M = 1, 2, 4, 8 models: obj_06 with api.PPFModel's defaults, then scaled and stretched synth.uv_sphere_mesh blobs sampled at different fractions
of their diameter (different sample counts, so different LDS sizes in one launch).  For every M the two routes alternate call by call in one
process (host clock around the synchronous calls, --calls after --warmup): api.ppf_vote_multi against M api.ppf_vote calls, and
api.generate_hypotheses_multi against M api.generate_hypotheses calls.  The single route is timed per model; its figure is the sum of the M
medians, with the sum of the minima and of the maxima beside it, and the median of the per-round totals.  Both routes must give the same bytes
(asserted).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_refine_amd import api, synth  # noqa: E402
from pose_accuracy import stats  # noqa: E402

# (n_lon, n_lat, scale, stretch, step as a fraction of the diameter) of the blobs behind obj_06
BLOBS = [(24, 16, 1.0, (1.0, 0.7, 0.45), 0.05), (10, 8, 1.0, (1.0, 0.8, 0.6), 0.07), (32, 20, 1.4, (0.6, 1.0, 0.8), 0.04), (16, 12, 0.7, (1.0, 0.5, 0.9), 0.09),
         (20, 14, 1.2, (0.8, 0.9, 1.0), 0.06), (28, 18, 0.9, (1.0, 0.6, 0.7), 0.045), (12, 10, 1.6, (0.5, 0.8, 1.0), 0.08)]


def blob_model(n_lon, n_lat, scale, stretch, fraction):
    tris = (synth.uv_sphere_mesh(n_lon, n_lat).astype(np.float64) * scale * np.array(stretch)).astype(np.float32)
    v = tris.reshape(-1, 3).astype(np.float64)
    return api.PPFModel(tris, step_mm=fraction * float(np.linalg.norm(v.max(0) - v.min(0))))


def sums(per_model):
    """The single route from its per-model samples: the sum of the medians (min, max), and the per-round totals."""
    s = [stats(ms) for ms in per_model]
    out = {k: round(sum(x[k] for x in s), 4) for k in ("median_ms", "min_ms", "max_ms")}
    out["round_total"] = stats([sum(r) for r in zip(*per_model)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--ref-stride", type=int, default=5)
    args = ap.parse_args()
    api.init(0)
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    depth = api.render_host(model, synth.scene_pose()[None], W, H, api.compute_proj(K, W, H))[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    models = [api.PPFModel(model).build()] + [blob_model(*b).build() for b in BLOBS]
    pts, nrm, n_scene = api.ppf_scene_points(scene, args.stride)
    n_refs = (n_scene - 1) // args.ref_stride + 1
    out = {"workload": "obj_06.ply at synth.scene_pose(), 640x480; models: obj_06, then blobs", "n_model": [len(m.points) for m in models],
           "cells": [len(m.points) * m.params.n_alpha for m in models], "n_entries": [m.n_entries for m in models], "stride": args.stride,
           "ref_stride": args.ref_stride, "n_scene": n_scene, "n_refs": n_refs, "calls": args.calls, "warmup_calls": args.warmup, "models": {}}
    for M in (1, 2, 4, 8):
        table = models[:M]
        vote_multi, vote_single, gen_multi, gen_single = [], [[] for _ in table], [], [[] for _ in table]
        for it in range(args.warmup + args.calls):
            keep = it >= args.warmup
            t0 = time.perf_counter()
            peaks, poses = api.ppf_vote_multi(table, pts, nrm, n_scene, 0, args.ref_stride, n_refs, 1)
            if keep:
                vote_multi.append((time.perf_counter() - t0) * 1e3)
            for k, m in enumerate(table):
                t0 = time.perf_counter()
                p1, q1 = api.ppf_vote(m, pts, nrm, n_scene, 0, args.ref_stride, n_refs, 1)
                if keep:
                    vote_single[k].append((time.perf_counter() - t0) * 1e3)
                assert peaks[k].tobytes() == p1.tobytes() and poses[k].tobytes() == q1.tobytes()
            t0 = time.perf_counter()
            idx, hyp, votes = api.generate_hypotheses_multi(table, scene, args.stride, args.ref_stride)
            if keep:
                gen_multi.append((time.perf_counter() - t0) * 1e3)
            for k, m in enumerate(table):
                t0 = time.perf_counter()
                h1, v1 = api.generate_hypotheses(m, scene, args.stride, args.ref_stride)
                if keep:
                    gen_single[k].append((time.perf_counter() - t0) * 1e3)
                assert hyp[idx == k].tobytes() == h1.tobytes() and votes[idx == k].tobytes() == v1.tobytes()
        out["models"][str(M)] = {"vote_multi": stats(vote_multi), "vote_single_sum": sums(vote_single), "generate_multi": stats(gen_multi),
                                 "generate_single_sum": sums(gen_single), "hypotheses": [int((idx == k).sum()) for k in range(M)]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
