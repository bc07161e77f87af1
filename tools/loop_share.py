#!/usr/bin/env python
"""Serial share of a pass of the resident loop (icp_loop_cu_kernel), from a measuring build of the library:

    PR_EXTRA_FLAGS=-DPR_LOOP_CU_PROBE=1 PR_BUILD_OUT=pose_refine_amd/lib/variants/probe.so python -m pose_refine_amd.build
    PR_LIB_PATH=pose_refine_amd/lib/variants/probe.so [PR_OPTS=loop_waves=8,...] python tools/loop_share.py [hypotheses]

Wavefront 0 of every workgroup sums ticks of the 100 MHz wall clock over the stretch between the two barriers of a pass (row sums + solve, the other
wavefronts wait) and over whole passes, and leaves both per hypothesis in the slot's partial buffer, which pr_loop_probe_read copies out.  Printed per
cloud size in blocks of points_per_block points: hypotheses, passes, microseconds per pass serial and whole, and their ratio.  The headline batch of
bench.py: 256 hypotheses of obj_06 at 640x480, 21 passes."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pose_refine_amd import _lib, api, synth

P = int(sys.argv[1]) if len(sys.argv) > 1 else 256
lib = _lib.load()
if not hasattr(lib, "pr_loop_probe_read"):
    sys.exit("this library was built without -DPR_LOOP_CU_PROBE=1")
api.init(0)
api.set_option("solve", 1)
for kv in filter(None, os.environ.get("PR_OPTS", "").split(",")):
    k, v = kv.split("=")
    api.set_option(k, int(v))
model = api.Model(os.path.join(ROOT, "tests/golden/obj_06.ply"))
K = synth.K_TEST
proj = api.compute_proj(K, 640, 480)
sd = api.render_host(model, synth.scene_pose()[None], 640, 480, proj)[0]
scene = api.Scene_projective().init_Scene_projective_cuda(sd, K)
poses = synth.hypotheses(P)
crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
STEPS = 8                                                           # both slots in turn as bench.py drives them; the last batch is measured
api.refine_submit(0, model, poses, 640, 480, proj, K, scene, crit)
for k in range(1, STEPS):
    api.refine_submit(k & 1, model, poses, 640, 480, proj, K, scene, crit)
    api.refine_wait((k - 1) & 1)
_, sizes = api.refine_wait((STEPS - 1) & 1)
out = np.zeros((P, 4), np.float32)
rc = lib.pr_loop_probe_read((STEPS - 1) & 1, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(P))
if rc != 0:
    sys.exit("pr_loop_probe_read failed: %d" % rc)
print("waves %d, LDS blocks %d, table bytes %d, resident batches %d" % tuple(
    api.get_option(n) for n in ("stat_loop_waves", "stat_loop_lds_blocks", "stat_loop_lds_tables", "stat_resident_batches")))
serial, total, passes, items = out.T.astype(np.float64)
tick_us = 0.01
print("blocks  hypotheses  passes  serial us/pass  pass us  serial share")
for nb in sorted(set((items // 4).astype(int))):
    m = (items // 4).astype(int) == nb
    s, t = serial[m].sum() / passes[m].sum() * tick_us, total[m].sum() / passes[m].sum() * tick_us
    print("%6d  %10d  %6.1f  %14.2f  %7.2f  %11.1f %%" % (nb, m.sum(), passes[m].mean(), s, t, 100.0 * s / t))
s, t = serial.sum() / passes.sum() * tick_us, total.sum() / passes.sum() * tick_us
print("   all  %10d  %6.1f  %14.2f  %7.2f  %11.1f %%" % (P, passes.mean(), s, t, 100.0 * s / t))
print("slowest hypothesis: %.1f us over %d passes" % (total.max() * tick_us, int(passes[total.argmax()])))
