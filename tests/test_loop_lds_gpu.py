"""GPU tests (-m gpu) of the resident loop's LDS image (option loop_lds_blocks): the first R blocks of every cloud stay in the workgroup's LDS over
the whole loop -- loaded from memory in pass 0, read, moved and written in LDS from then on -- while the other blocks move through memory as before.
Same source per point, same tree, same solve: T, fitness, rmse and cloud sizes must be byte-identical to the unchanged multi-launch route
(resident_loop = 0), which is the reference of every case, for loop_lds_blocks = 0, 1, 2 and -1 on both slots.  Read-only option
stat_loop_lds_blocks (the R of the most recent resident launch) proves that no case quietly ran with R = 0, and stat_resident_batches that the
batches really took the resident route."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H
from test_tight_box_gpu import near_plane_pose, same
from test_resident_loop_gpu import NONE, PPB, ROI_SMALL, batch, crit, resident_batches

pytestmark = [pytest.mark.gpu, pytest.mark.device_solve]

f32 = np.float32
CAPS = (0, 1, 2, -1)
LDS_TOTAL, LDS_BUDGET = 160 << 10, 64 << 10


def lds_blocks():
    return api.get_option("stat_loop_lds_blocks")


def fit(nblk, ppb):
    """R of a plan of nblk blocks without a cap: rows of 128 bytes, four per block, a 256-byte header, then whole blocks of 12-byte points."""
    return min(nblk, (LDS_TOTAL - (nblk * 512 + 256)) // (ppb * 12))


def caps_match(run, caps=CAPS, expect=2):
    """run(slot) -> (records, sizes).  Reference with resident_loop = 0 (two batches first: the ordered copy and the vertex list are made on a
    buffer's second batch); then, for every cap, one batch per slot on the resident route; then the multi-launch loop again.  `expect`: by how
    much the two batches of a cap advance stat_resident_batches.  Returns the reference and {cap: R the launches ran with}."""
    default = api.get_option("loop_lds_blocks")
    used = {}
    try:
        api.set_option("resident_loop", 0)
        run(0)
        ref = run(1)
        api.set_option("resident_loop", 1)
        for cap in caps:
            api.set_option("loop_lds_blocks", cap)
            before = resident_batches()
            rs = []
            for slot in (0, 1):
                assert same(run(slot), ref), f"loop_lds_blocks={cap}, slot {slot}"
                rs.append(lds_blocks())
            assert resident_batches() == before + expect
            assert rs[0] == rs[1]
            used[cap] = rs[0]
        api.set_option("resident_loop", 0)
        assert same(run(0), ref)
    finally:
        api.set_option("resident_loop", 1)
        api.set_option("loop_lds_blocks", default)
    if expect:
        most = used[-1]
        assert used[0] == 0 and most > 0, used
        for cap in caps:
            if cap > 0:
                assert used[cap] == min(cap, most), used
    return ref, used


def slots_match(m, poses, frame, scene, criteria, roi=NONE, caps=CAPS, expect=2):
    return caps_match(lambda slot: batch(slot, m, poses, frame, scene, criteria, roi), caps, expect)


@pytest.fixture(scope="module")
def frame(scenario):
    return W, H, scenario["proj"], scenario["K"]


def test_the_option_reads_back(gpu):
    default = api.get_option("loop_lds_blocks")
    try:
        for v, back in ((3, 3), (0, 0), (-1, -1), (-7, -1)):
            api.set_option("loop_lds_blocks", v)
            assert api.get_option("loop_lds_blocks") == back
    finally:
        api.set_option("loop_lds_blocks", default)


@pytest.mark.parametrize("iters", [0, 1, 2, 6])
def test_fixed_iterations(gpu, model, frame, gscenes, iters):
    """Thresholds 0: every hypothesis runs iters + 1 passes.  0 is the score-only pass alone, which fills LDS and never reads it; 1 the first fill
    of LDS without a transform and the first LDS -> LDS pass (score-only, with a transform); 2 the second LDS -> LDS pass; 6 the loop."""
    (res, sizes), used = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(iters))
    # the plan's blocks come from the largest pixel box, which the test does not see: rows within 64 KiB leave 96 KiB, two blocks of 36 864 bytes
    # at least, and five (184 320 bytes) never fit; whatever R is, every cloud here is longer than the image
    assert 2 <= used[-1] <= 4
    assert sizes.min() > 4 * PPB
    if iters:
        assert not np.array_equal(res["T"][0].reshape(4, 4), np.eye(4, dtype=f32))


def test_partial_residency(gpu, model, frame, gscenes):
    """loop_lds_blocks = 1 and 2: only wavefronts 0-3, then 0-7, hold an item of the LDS image; the others hold none."""
    (res, sizes), used = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), caps=(1, 2, 0, -1))
    assert used[1] == 1 and used[2] == 2
    assert sizes.min() > 2 * PPB


ROI_WIDE = (200, 110, 250, 260)


def test_four_blocks_resident(gpu, model, frame, gscenes):
    """A window of 65 000 pixels bounds every box to 22 blocks: four blocks fit beside their rows, items 0 .. 15 -- the first item of every
    wavefront is in LDS, and clouds longer than four blocks have the rest in memory."""
    window_blocks = -(-ROI_WIDE[2] * ROI_WIDE[3] // PPB)
    assert fit(window_blocks, PPB) == 4 and fit(4, PPB) == 4
    (res, sizes), used = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), roi=ROI_WIDE)
    assert used[-1] == 4, used
    assert (sizes > 4 * PPB).any(), sizes


def test_many_small_blocks(gpu, model, frame, gscenes):
    """1024 points per block: a cloud has more blocks than fit, and more resident blocks than four -- a wavefront takes items of the LDS image
    and items in memory in the same pass."""
    try:
        api.set_option("points_per_block", 1024)
        (res, sizes), used = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6))
        r = used[-1]
        assert 0 < r * 1024 < sizes.min()
        assert r > 4                                                 # items 16 .. 4 r - 1: a second resident item per wavefront
    finally:
        api.set_option("points_per_block", PPB)


def test_whole_cloud_resident(gpu, model, frame, gscenes):
    """A window small enough that every cloud is under one block, all of it in LDS: a partial last block, lanes past the end (they read the
    cloud's last point from the image), wavefronts with an item without a point or with none at all."""
    (res, sizes), used = slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), roi=ROI_SMALL)
    assert used[-1] >= 1
    assert sizes.max() > 0 and sizes.max() < PPB
    assert ((sizes > 0) & (sizes < 768)).any(), sizes
    assert (sizes >= 768).any(), sizes


ROI_MID = (270, 170, 100, 100)


def test_block_boundary(gpu, model, frame, gscenes):
    """The edge between the LDS image and memory: with R blocks resident, one cloud of exactly R blocks (its partial last block is the image's
    last) and one of R + 1 (its last block is the only one in memory).  1024 points per block and a window, so that the clouds of a batch differ
    by whole blocks; R is taken from their sizes and set as the cap."""
    poses = synth.hypotheses(32)
    try:
        api.set_option("points_per_block", 1024)
        api.set_option("resident_loop", 0)
        batch(0, model, poses, frame, gscenes["proj"], crit(2), ROI_MID)
        sizes = batch(1, model, poses, frame, gscenes["proj"], crit(2), ROI_MID)[1]
        blocks = -(-sizes.astype(np.int64) // 1024)
        window_blocks = -(-ROI_MID[2] * ROI_MID[3] // 1024)
        pairs = [r for r in range(1, fit(window_blocks, 1024) + 1) if (blocks == r).any() and (blocks == r + 1).any()]
        assert pairs, np.sort(blocks)
        r = pairs[-1]
        (res, sizes2), used = slots_match(model, poses, frame, gscenes["proj"], crit(6), roi=ROI_MID, caps=(0, 1, 2, -1, r))
        assert np.array_equal(sizes2, sizes)
        assert used[r] == r
        assert (blocks == r).any() and (blocks == r + 1).any()
    finally:
        api.set_option("resident_loop", 1)
        api.set_option("points_per_block", PPB)


def test_second_round_workgroups(gpu, model, frame, gscenes):
    """257 hypotheses: one workgroup more than the chip has compute units -- a workgroup starts on LDS that another hypothesis has filled, and
    reads only what it stored itself."""
    slots_match(model, synth.hypotheses(257), frame, gscenes["proj"], crit(2))


def test_default_criteria(gpu, model, frame, gscenes):
    """The reference's default criteria: hypotheses leave the loop at different passes."""
    slots_match(model, synth.hypotheses(8), frame, gscenes["proj"], api.ICPConvergenceCriteria())


def test_a_hypothesis_that_renders_nothing(gpu, model, frame, gscenes):
    """Wholly outside the frame between two that render: its workgroup returns ahead of every barrier and touches no LDS."""
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[3, 0, 3] += f32(2000.0)
    (res, sizes), used = slots_match(model, poses, frame, gscenes["proj"], crit(6))
    assert sizes[3] == 0 and np.array_equal(res["T"][3].reshape(4, 4), np.eye(4, dtype=f32))
    assert sizes[2] > 0 and sizes[4] > 0


def test_two_sub_batches(gpu, model, frame, gscenes):
    try:
        api.set_option("sub_batch", 32)
        slots_match(model, synth.hypotheses(40), frame, gscenes["proj"], crit(2), expect=4)
    finally:
        api.set_option("sub_batch", 512)


def test_near_plane_pose(gpu, model, scenario, frame, gscenes):
    """A hypothesis with a vertex at the camera plane has the whole frame for its box: at 3072 points per block the plan holds W H / 3072 blocks,
    whose rows take most of the kernel's 64 KiB.  The batch stays resident with fewer than four blocks in LDS; were the rows over 64 KiB, it
    would have to take the multi-launch loop as before."""
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[5] = near_plane_pose(scenario["tris"], poses[5])
    assert np.array_equal(api.tight_box(scenario["tris"], poses[5], W, H, scenario["proj"])[0], [0, 0, W - 1, H - 1])
    nblk = -(-W * H // PPB)
    if nblk * 512 + 256 > LDS_BUDGET:
        (res, sizes), used = slots_match(model, poses, frame, gscenes["proj"], crit(2), expect=0)
    else:
        (res, sizes), used = slots_match(model, poses, frame, gscenes["proj"], crit(2))
        assert 0 < used[-1] < 4
        assert used[-1] == fit(nblk, PPB)
    assert sizes[0] > 0
