#!/usr/bin/env python
"""What a scene from a point cloud (api.Scene_nn().init_Scene_nn_cloud / pr_scene_nn_from_cloud_dev) costs, next to the depth route's device
preparation (pr_scene_nn_prepare_dev) of the same frames: the bench's scene (the object alone) and a frame-filling one (the object in front of a
wall, 307 k points), at k = 8, 16, 32.  Host clocks around synchronous calls, after warm-up; median / min / max ms of --calls calls.  Per scene:
  kdtree_prepare_dev        the depth route: normals by the stencil, gather, tree build
  kdtree_build_dev          the tree build alone on the bare points (in the order the depth route's builder meets them)
and per k:
  from_cloud                pr_scene_nn_from_cloud_dev into buffers that exist: tree build, traversal records (make_scene), k-NN walk + normals
  normals                   pr_cloud_normals_dev on the built scene, its traversal records derived: the kernel, one memset, one read-back
  knn                       pr_cloud_knn_dev on the same scene: the walk and the n x k lists written out
The one step runs in a child process of its own under its own time limit.  One JSON line.

    python tools/cloud_time.py [--calls 5] [--warmup 2] [--k 8,16,32] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pose_refine_amd import api, synth  # noqa: E402

W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def timed(fn):
    api.sync(); t = time.perf_counter(); r = fn(); api.sync()
    return (time.perf_counter() - t) * 1e3, r


def repeat(args, fn, before=None):
    ms = []
    for _ in range(args.warmup + args.calls):
        if before:
            before()
        ms.append(timed(fn)[0])
    return stats(ms[args.warmup:])


def frames():
    model = api.Model(os.path.join(ROOT, "tests", "golden", "obj_06.ply"))
    obj = api.render_host(model, synth.scene_pose()[None], W, H, api.compute_proj(K, W, H))[0]
    yy, xx = np.mgrid[0:H, 0:W]
    wall = (900 + 0.05 * xx + 0.03 * yy + 3.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)).astype(np.int32)       # tools/grid_time.py's frame-filling scene
    return (("object_alone", obj.astype(np.int32)), ("object_and_wall", np.where(obj > 0, obj, wall).astype(np.int32)))


def step_cost(args):
    lib, C = api._lib.load(), api.C
    out = {}
    for name, depth in frames():
        dev = api.DeviceVector.from_host(depth.reshape(-1))
        nn = api.Scene_nn()
        r = {"points": int((depth > 0).sum()), "kdtree_prepare_dev": repeat(args, lambda: nn.init_Scene_nn_device(dev, K, W, H))}
        dense = api.Scene_projective().init_Scene_projective_cuda(depth, K).pcd_host
        src = api.DeviceVector.from_host(np.ascontiguousarray(dense[dense[:, 2] > 0]).reshape(-1))          # the bare points, pixel order
        n = src.size() // 3
        pcd, nrm, nodes = api.DeviceVector(n * 3, np.float32), api.DeviceVector(n * 3, np.float32), api.DeviceVector(2 * n + 1, api.KDNODE)
        nnodes = C.c_uint32()
        fresh = lambda: api.check(lib.pr_memcpy_d2d(pcd.data(), src.data(), n * 12))                        # (the build reorders in place: not timed)
        r["kdtree_build_dev"] = repeat(args, lambda: api.check(lib.pr_kdtree_build_dev(pcd.data(), nrm.data(), n, 10, nodes.data(), 2 * n + 1, C.byref(nnodes))), fresh)
        for k in args.k:
            p, counts = api.CloudParams(k=k), api.CloudCounts()
            rk = {"from_cloud": repeat(args, lambda: api.check(lib.pr_scene_nn_from_cloud_dev(pcd.data(), n, 10, C.addressof(p), nrm.data(), nodes.data(), 2 * n + 1,
                                                                                                C.byref(nnodes), C.addressof(counts))), fresh)}
            scene = api.Scene_nn()
            scene.pcd_buffer, scene.normal_buffer, scene.nodes, scene._n_points, scene._n_nodes, scene.camera = pcd, nrm, nodes, n, nnodes.value, None
            d = scene.desc()
            rk["normals"] = repeat(args, lambda: api.check(lib.pr_cloud_normals_dev(C.addressof(d), C.addressof(p), nrm.data(), None, C.addressof(counts))))
            idx, d2, cnt = api.DeviceVector(n * k, np.uint32), api.DeviceVector(n * k, np.float32), api.DeviceVector(n, np.uint32)
            rk["knn"] = repeat(args, lambda: api.check(lib.pr_cloud_knn_dev(C.addressof(d), C.addressof(p), idx.data(), d2.data(), cnt.data())))
            rk["list_bytes"] = n * k * 8 + n * 4
            rk["counts"] = api._cloud_counts(counts)
            r[f"k{k}"] = rk
            del idx, d2, cnt
        out[name] = r
    return {"calls": args.calls, "warmup_calls": args.warmup, "max_leaf": 10, "scenes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=lambda s: [int(v) for v in s.split(",")], default=[8, 16, 32])
    ap.add_argument("--step", choices=("cost",), default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds the step may take")
    args = ap.parse_args()
    if args.step is None:                                          # the driver: the step in a fresh process under `timeout`
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", "cost", "--calls", str(args.calls),
               "--warmup", str(args.warmup), "--k", ",".join(str(k) for k in args.k)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(json.dumps({"step": "cost", "failed": p.returncode, "stderr": p.stderr[-2000:]}), flush=True)
            sys.exit(1)
        print(p.stdout.strip().splitlines()[-1], flush=True)
        return
    api.init(0)
    print(json.dumps({"cost": step_cost(args)}), flush=True)


if __name__ == "__main__":
    main()
