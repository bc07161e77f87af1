"""GPU tests (-m gpu) of the asynchronous path's banded depth boxes (option box_bands): four consecutive image rows of a hypothesis' box are
interleaved column by column, so that the raster's depth atomics touch fewer 64-byte segments.  A depth image is a per-pixel minimum and the
clouds are emitted in the same order, so every batch must be byte-identical with the option off and on -- T, fitness, rmse and cloud sizes.
Read-only option stat_band_batches counts the batches that really ran on banded boxes, so that no case passes by quietly staying row-major."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H
from test_tight_box_gpu import near_plane_pose, same

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0, 0)
f32 = np.float32
CRIT = api.ICPConvergenceCriteria(0.0, 0.0, 6)
CRIT2 = api.ICPConvergenceCriteria(0.0, 0.0, 2)


def band_batches():
    return api.get_option("stat_band_batches")


def batch(slot, m, poses, frame, scene, crit, roi=NONE):
    w, h, proj, K = frame
    api.refine_submit(slot, m, poses, w, h, proj, K, scene, crit, roi=roi)
    return api.refine_wait(slot)


def rows_and_bands_match(m, poses, frame, scene, crit, roi=NONE, expect_bands=2):
    """Reference with box_bands = 0 (two batches first: the ordered copy and the vertex list are made on a buffer's second batch), then one
    batch per slot with box_bands = 1, then row-major again.  Returns the reference."""
    try:
        api.set_option("box_bands", 0)
        before = band_batches()
        batch(0, m, poses, frame, scene, crit, roi)
        ref = batch(1, m, poses, frame, scene, crit, roi)
        assert band_batches() == before
        api.set_option("box_bands", 1)
        for slot in (0, 1):
            assert same(batch(slot, m, poses, frame, scene, crit, roi), ref), f"box_bands=1, slot {slot}"
        assert band_batches() == before + expect_bands
        api.set_option("box_bands", 0)
        assert same(batch(0, m, poses, frame, scene, crit, roi), ref)
    finally:
        api.set_option("box_bands", 1)
    return ref


@pytest.fixture(scope="module")
def frame(scenario):
    return W, H, scenario["proj"], scenario["K"]


def test_the_option_defaults_to_bands(gpu):
    assert api.get_option("box_bands") == 1


@pytest.mark.device_solve
def test_projective_scene(gpu, model, frame, gscenes):
    ref = rows_and_bands_match(model, synth.hypotheses(8), frame, gscenes["proj"], CRIT)
    assert ref[1].min() > 0


@pytest.mark.device_solve
def test_kdtree_scene(gpu, model, frame, gscenes):
    ref = rows_and_bands_match(model, synth.hypotheses(8), frame, gscenes["nn"], CRIT)
    assert ref[1].min() > 0


def test_host_solve_stays_on_the_synchronous_path(gpu, model, frame, gscenes):
    """Host solve: the slots' helper threads run the synchronous path, which keeps its row-major boxes -- no batch counts as banded."""
    rows_and_bands_match(model, synth.hypotheses(8), frame, gscenes["proj"], CRIT, expect_bands=0)


@pytest.mark.device_solve
def test_roi(gpu, model, frame, gscenes):
    ref = rows_and_bands_match(model, synth.hypotheses(8), frame, gscenes["proj"], CRIT, roi=(250, 150, 180, 160))
    assert ref[1].max() > 0


@pytest.mark.device_solve
@pytest.mark.parametrize("n", [1, 257])                            # 257: the offset scan carries over its 256-entry chunk
def test_batch_sizes(gpu, model, frame, gscenes, n):
    rows_and_bands_match(model, synth.hypotheses(n), frame, gscenes["proj"], CRIT2)


@pytest.mark.device_solve
def test_offsets_restart_at_every_sub_batch(gpu, model, frame, gscenes):
    try:
        api.set_option("sub_batch", 32)
        rows_and_bands_match(model, synth.hypotheses(40), frame, gscenes["proj"], CRIT2)
    finally:
        api.set_option("sub_batch", 512)


@pytest.mark.device_solve
@pytest.mark.parametrize("tight", [0, 1])
@pytest.mark.parametrize("order", [0, 1])
def test_with_and_without_tight_boxes_and_the_ordered_mesh(gpu, model, frame, gscenes, tight, order):
    """Loose boxes keep the host's offsets, tight ones get theirs from box_pack_offsets_kernel; the raster reads the caller's buffer or the copy."""
    try:
        api.set_option("tight_box", tight)
        api.set_option("mesh_order", order)
        before = api.get_option("stat_tight_batches")
        ref = rows_and_bands_match(model, synth.hypotheses(8), frame, gscenes["proj"], CRIT)
        assert ref[1].min() > 0
        assert (api.get_option("stat_tight_batches") > before) == bool(tight)
    finally:
        api.set_option("tight_box", 1)
        api.set_option("mesh_order", 1)


@pytest.mark.device_solve
def test_special_poses(gpu, model, scenario, frame, gscenes):
    """Half out of the frame; wholly outside (empty box, empty cloud, identity result); a vertex at the camera plane (the loose full-frame box)."""
    tris = scenario["tris"]
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[1, 0, 3] += f32(150.0)
    poses[3, 0, 3] += f32(2000.0)
    poses[5] = near_plane_pose(tris, poses[5])
    tight, loose = zip(*(api.tight_box(tris, poses[i], W, H, scenario["proj"]) for i in (1, 3, 5)))
    assert tight[0][2] == W - 1 and tight[0][0] > 0
    assert tight[1][2] < tight[1][0]
    assert np.array_equal(tight[2], [0, 0, W - 1, H - 1])
    res, sizes = rows_and_bands_match(model, poses, frame, gscenes["proj"], CRIT)
    assert sizes[3] == 0 and np.array_equal(res["T"][3].reshape(4, 4), np.eye(4, dtype=f32))
    assert sizes[1] > 0 and sizes[5] > 0


@pytest.mark.device_solve
def test_frame_whose_sides_are_no_multiples_of_four(gpu, model, scenario):
    """161 x 123: the last band of a box that reaches the frame's last row has a row past the frame, and the widths are odd.  Hypothesis 5 has a
    vertex at the camera plane, so its box is the whole frame; hypotheses 2 and 4 are pushed to where their boxes reach the frame's last and first
    image row."""
    w, h = 161, 123
    K = (synth.K_TEST.reshape(3, 3) * np.array([[0.25], [0.25], [1.0]], f32)).astype(f32).reshape(9)
    K[2], K[5] = f32(80.0), f32(61.0)
    proj = api.compute_proj(K, w, h)
    scene = api.Scene_projective().init_Scene_projective_cuda(api.render_host(model, synth.scene_pose()[None], w, h, proj)[0], K, w, h)
    tris = scenario["tris"]
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[2, 1, 3] += f32(120.0)
    poses[4, 1, 3] -= f32(120.0)
    poses[5] = near_plane_pose(tris, poses[5])
    boxes = [api.tight_box(tris, p, w, h, proj)[0] for p in poses]
    assert np.array_equal(boxes[5], [0, 0, w - 1, h - 1])
    assert boxes[2][1] == 0 and 0 < boxes[2][3] < h - 1               # raster y = 0 is image row h - 1: its band has a row past the frame
    assert boxes[4][3] == h - 1 and 0 < boxes[4][1]
    res, sizes = rows_and_bands_match(model, poses, (w, h, proj, K), scene, CRIT)
    assert sizes[0] > 0 and sizes[2] > 0 and sizes[4] > 0
