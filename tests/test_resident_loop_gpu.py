"""GPU tests (-m gpu) of the asynchronous path's resident loop (option resident_loop): all passes of a sub-batch in one launch, one 1024-lane
workgroup per hypothesis (icp_loop_cu_kernel), instead of one launch per pass and pose group.  Same per-point source, same summation tree, same
solve: every batch must be byte-identical with the option off and on -- T, fitness, rmse and cloud sizes.  The reference of every case is the
unchanged multi-launch route (resident_loop = 0), run before and after.  Read-only option stat_resident_batches counts the sub-batches that
really ran resident, so that no case passes by quietly staying on the multi-launch route -- and none that must stay there leaves it."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H
from test_tight_box_gpu import near_plane_pose, same

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0, 0)
f32 = np.float32
PPB = 3072                                                          # the library's points_per_block


def crit(n):
    return api.ICPConvergenceCriteria(0.0, 0.0, n)


def resident_batches():
    return api.get_option("stat_resident_batches")


def batch(slot, m, poses, frame, scene, criteria, roi=NONE):
    w, h, proj, K = frame
    api.refine_submit(slot, m, poses, w, h, proj, K, scene, criteria, roi=roi)
    return api.refine_wait(slot)


def loops_match(run, expect):
    """run(slot) -> (records, sizes).  Reference with resident_loop = 0 (two batches first: the ordered copy and the vertex list are made on a
    buffer's second batch), then one batch per slot with resident_loop = 1, then the multi-launch loop again.  `expect`: by how much the two
    resident_loop = 1 batches must advance stat_resident_batches.  Returns the reference."""
    try:
        api.set_option("resident_loop", 0)
        before = resident_batches()
        run(0)
        ref = run(1)
        assert resident_batches() == before
        api.set_option("resident_loop", 1)
        for slot in (0, 1):
            assert same(run(slot), ref), f"resident_loop=1, slot {slot}"
        assert resident_batches() == before + expect
        api.set_option("resident_loop", 0)
        assert same(run(0), ref)
        assert resident_batches() == before + expect
    finally:
        api.set_option("resident_loop", 1)
    return ref


def slots_match(m, poses, frame, scene, criteria, roi=NONE, expect=2):
    return loops_match(lambda slot: batch(slot, m, poses, frame, scene, criteria, roi), expect)


@pytest.fixture(scope="module")
def frame(scenario):
    return W, H, scenario["proj"], scenario["K"]


def test_the_option_defaults_to_resident(gpu):
    assert api.get_option("resident_loop") == 1


@pytest.mark.device_solve
def test_one_hypothesis_score_only_pass(gpu, model, frame, gscenes):
    """The smallest run: one workgroup, max_iteration = 0 -- the score-only pass alone, no transform, no update handed over."""
    res, sizes = slots_match(model, synth.hypotheses(1), frame, gscenes["proj"], crit(0))
    assert sizes[0] > 0 and res["fitness"][0] > 0


@pytest.mark.device_solve
@pytest.mark.parametrize("iters", [0, 1, 2, 6])
def test_fixed_iterations(gpu, model, frame, gscenes, iters):
    """Thresholds 0: every hypothesis runs iters + 1 passes.  0 is the score-only pass alone; 1 pins the first transform and the hand-over of the
    update through LDS; 2 the second hand-over; 6 the loop."""
    res, sizes = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(iters))
    assert sizes.min() > 0
    if iters:
        assert not np.array_equal(res["T"][0].reshape(4, 4), np.eye(4, dtype=f32))


@pytest.mark.device_solve
def test_default_criteria(gpu, model, frame, gscenes):
    """The reference's default criteria: hypotheses leave the loop at different passes (their workgroups end, nobody waits for them)."""
    slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], api.ICPConvergenceCriteria())


@pytest.mark.device_solve
@pytest.mark.parametrize("n", [1, 257])                            # 257: one workgroup more than the chip has compute units
def test_batch_sizes(gpu, model, frame, gscenes, n):
    slots_match(model, synth.hypotheses(n), frame, gscenes["proj"], crit(2))


@pytest.mark.device_solve
@pytest.mark.parametrize("ppb", [1024, 3072])
def test_points_per_block(gpu, model, frame, gscenes, ppb):
    """1024: a cloud has more blocks than the workgroup has wavefronts -- every wavefront takes several items, the block-order sum has many terms.
    3072: fewer items than four per wavefront, the last round of items is partial."""
    try:
        api.set_option("points_per_block", ppb)
        res, sizes = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6))
        items = 4 * -(-sizes.astype(np.int64) // ppb)
        if ppb == 1024:
            assert items.min() > 2 * 16
        else:
            assert (items % 16 != 0).any() and items.min() > 16
    finally:
        api.set_option("points_per_block", PPB)


ROI_SMALL = (300, 200, 40, 60)


@pytest.mark.device_solve
def test_roi(gpu, model, frame, gscenes):
    """A window small enough that every cloud is under one block: some wavefronts of the workgroup have an item without a point or none at all."""
    res, sizes = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), roi=ROI_SMALL)
    assert sizes.max() > 0 and sizes.max() < PPB
    assert ((sizes > 0) & (sizes < 768)).any(), sizes                # under one wavefront's 768 points of a block
    assert (sizes >= 768).any(), sizes


@pytest.mark.device_solve
def test_a_hypothesis_that_renders_nothing(gpu, model, frame, gscenes):
    """Wholly outside the frame (empty cloud, skipped: its workgroup returns at once, identity result) between two that render."""
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[3, 0, 3] += f32(2000.0)
    res, sizes = slots_match(model, poses, frame, gscenes["proj"], crit(6))
    assert sizes[3] == 0 and np.array_equal(res["T"][3].reshape(4, 4), np.eye(4, dtype=f32))
    assert sizes[2] > 0 and sizes[4] > 0


@pytest.mark.device_solve
def test_two_sub_batches(gpu, model, frame, gscenes):
    try:
        api.set_option("sub_batch", 32)
        slots_match(model, synth.hypotheses(40), frame, gscenes["proj"], crit(2), expect=4)
    finally:
        api.set_option("sub_batch", 512)


# ---- routes that keep the multi-launch loop: same bytes as before, the counter stands still ------------------------------------------------
@pytest.mark.device_solve
def test_kdtree_scene_keeps_the_multi_launch_loop(gpu, model, frame, gscenes):
    ref = slots_match(model, synth.hypotheses(8), frame, gscenes["nn"], crit(6), expect=0)
    assert ref[1].min() > 0


def test_host_solve_keeps_the_multi_launch_loop(gpu, model, frame, gscenes):
    slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), expect=0)


@pytest.mark.device_solve
def test_robust_weight_keeps_the_multi_launch_loop(gpu, model, frame, gscenes):
    w, h, proj, K = frame
    rb = api.Robust(api.ROBUST_HUBER, 0.005)
    loops_match(lambda slot: api.refine_batch(model, synth.hypotheses(8), w, h, proj, K, gscenes["proj"], crit(6), robust=rb), 0)


@pytest.mark.device_solve
def test_timed_calls_keep_the_multi_launch_loop(gpu, model, frame, gscenes):
    """profile = 1: every launch of the loop carries events, so the loop keeps its launches."""
    try:
        api.set_option("profile", 1)
        slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), expect=0)
    finally:
        api.set_option("profile", 0)


@pytest.mark.device_solve
def test_over_the_lds_budget_falls_back(gpu, model, scenario, frame, gscenes):
    """A hypothesis with a vertex at the camera plane has the whole frame for its box: at 1024 points per block the plan holds 300 blocks, 1200 rows
    of 128 bytes -- over the kernel's 64 KiB.  The batch takes the multi-launch loop."""
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[5] = near_plane_pose(scenario["tris"], poses[5])
    assert np.array_equal(api.tight_box(scenario["tris"], poses[5], W, H, scenario["proj"])[0], [0, 0, W - 1, H - 1])
    try:
        api.set_option("points_per_block", 1024)
        res, sizes = slots_match(model, poses, frame, gscenes["proj"], crit(2), expect=0)
        assert sizes[0] > 0
    finally:
        api.set_option("points_per_block", PPB)
