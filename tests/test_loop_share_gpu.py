"""GPU tests (-m gpu) of the resident loop's two sharing options.  loop_lds_tables: the scene's colf / rowf tables are copied once per hypothesis
into the workgroup's LDS and two of the three gathers per point and pass read the copy.  loop_waves: the loop as an 8-wave workgroup, two to a
compute unit, instead of a 16-wave one.  Same source per point, same tree, same solve: T, fitness, rmse and cloud sizes must be byte-identical to
the unchanged multi-launch route (resident_loop = 0), which every case runs before and after, for every form on both slots.  The read-only options
stat_resident_batches, stat_loop_waves and stat_loop_lds_tables prove that no case passed by quietly running another form.

loop_lds_tables = 1 puts the tables in LDS whenever they fit beside rows and header -- they do in every plan here, at both limits -- so its stat is
known without the plan; -1, the default, is 1 for the 8-wave form and 0 for the 16-wave one."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H
from test_tight_box_gpu import same
from test_resident_loop_gpu import PPB, ROI_SMALL, batch, crit, resident_batches

pytestmark = [pytest.mark.gpu, pytest.mark.device_solve]

f32 = np.float32
WAVES = (16, 8)
OPTIONS = ("loop_waves", "loop_lds_tables", "loop_lds_blocks")


def table_bytes(w, h):
    return 4 * ((w + h + 3) // 4 * 4)


def stats():
    return api.get_option("stat_loop_waves"), api.get_option("stat_loop_lds_tables"), api.get_option("stat_loop_lds_blocks")


def forms_match(run, forms, size=(W, H), expect=2):
    """run(slot) -> (records, sizes).  Reference with resident_loop = 0 (two batches first: the ordered copy and the vertex list are made on a
    buffer's second batch); then, for every form (waves, tables, blocks), one batch per slot on the resident route; then the multi-launch loop
    again.  `expect`: by how much the two batches of a form advance stat_resident_batches.  Returns the reference."""
    defaults = [api.get_option(n) for n in OPTIONS]
    full = table_bytes(*size)
    try:
        api.set_option("resident_loop", 0)
        run(0)
        ref = run(1)
        api.set_option("resident_loop", 1)
        for waves, tables, blocks in forms:
            for n, v in zip(OPTIONS, (waves, tables, blocks)):
                api.set_option(n, v)
            before = resident_batches()
            for slot in (0, 1):
                assert same(run(slot), ref), f"loop_waves={waves}, loop_lds_tables={tables}, loop_lds_blocks={blocks}, slot {slot}"
                got_waves, got_tables, got_blocks = stats()
                assert got_waves == waves
                assert got_tables == (full if tables == 1 or (tables == -1 and waves == 8) else 0)
                if blocks == 0:
                    assert got_blocks == 0
            assert resident_batches() == before + expect
        api.set_option("resident_loop", 0)
        assert same(run(0), ref)
    finally:
        api.set_option("resident_loop", 1)
        for n, v in zip(OPTIONS, defaults):
            api.set_option(n, v)
    return ref


CROSS = [(w, t, b) for w in WAVES for t in (0, 1) for b in (0, -1)]
EIGHT = [(8, t, -1) for t in (0, 1, -1)]


@pytest.fixture(scope="module")
def frame(scenario):
    return W, H, scenario["proj"], scenario["K"]


def test_the_options_read_back(gpu, model, frame, gscenes):
    defaults = [api.get_option(n) for n in OPTIONS]
    try:
        assert defaults[0] == 0 and defaults[1] == -1
        for v in (8, 16, 0):
            api.set_option("loop_waves", v)
            assert api.get_option("loop_waves") == v
        for v in (4, 12, 32, -1):                                   # refused: the option keeps its value
            with pytest.raises(Exception):
                api.set_option("loop_waves", v)
            assert api.get_option("loop_waves") == 0
        for v, back in ((0, 0), (1, 1), (-1, -1), (7, 1), (-3, -1)):   # clamped
            api.set_option("loop_lds_tables", v)
            assert api.get_option("loop_lds_tables") == back
        api.set_option("loop_lds_tables", defaults[1])
        # eight hypotheses cannot fill the chip: the library's choice is the 16-wave form
        before = resident_batches()
        batch(0, model, synth.hypotheses(8), frame, gscenes["proj"], crit(1))
        assert resident_batches() == before + 1 and api.get_option("stat_loop_waves") == 16 and api.get_option("stat_loop_lds_tables") == 0
    finally:
        for n, v in zip(OPTIONS, defaults):
            api.set_option(n, v)


def test_one_hypothesis_score_only_pass(gpu, model, frame, gscenes):
    """One workgroup, max_iteration = 0: the table fill and the score-only pass alone, no update handed over."""
    res, sizes = forms_match(lambda slot: batch(slot, model, synth.hypotheses(1), frame, gscenes["proj"], crit(0)), CROSS)
    assert sizes[0] > 0 and res["fitness"][0] > 0


@pytest.mark.parametrize("iters", [1, 2, 6])
def test_fixed_iterations(gpu, model, frame, gscenes, iters):
    """Thresholds 0: every hypothesis runs iters + 1 passes -- fill, hand-over and loop in every form."""
    res, sizes = forms_match(lambda slot: batch(slot, model, synth.hypotheses(8), frame, gscenes["proj"], crit(iters)), CROSS)
    assert sizes.min() > 4 * PPB
    assert not np.array_equal(res["T"][0].reshape(4, 4), np.eye(4, dtype=f32))


def test_many_items(gpu, model, frame, gscenes):
    """1024 points per block on eight wavefronts: more than two items per wavefront, items of the LDS image and items in memory in one
    wavefront, a block-order sum of many terms."""
    try:
        api.set_option("points_per_block", 1024)
        res, sizes = forms_match(lambda slot: batch(slot, model, synth.hypotheses(8), frame, gscenes["proj"], crit(6)), EIGHT)
        assert (4 * -(-sizes.astype(np.int64) // 1024)).min() > 2 * 8
    finally:
        api.set_option("points_per_block", PPB)


def test_few_items(gpu, model, frame, gscenes):
    """A small window: clouds under 768 points -- wavefronts without an item still fill the tables and meet both barriers of every pass."""
    res, sizes = forms_match(lambda slot: batch(slot, model, synth.hypotheses(8), frame, gscenes["proj"], crit(6), ROI_SMALL), EIGHT + [(16, 1, -1)])
    assert ((sizes > 0) & (sizes < 768)).any(), sizes


def test_default_criteria(gpu, model, frame, gscenes):
    """The reference's default criteria: workgroups that share a compute unit leave the loop at different passes."""
    forms_match(lambda slot: batch(slot, model, synth.hypotheses(8), frame, gscenes["proj"], api.ICPConvergenceCriteria()), EIGHT)


@pytest.mark.parametrize("n", [257, 513])
def test_more_than_fits(gpu, model, frame, gscenes, n):
    """257: more workgroups than compute units, so some compute units hold two at once.  513: more 8-wave workgroups than a chip of 256 compute
    units holds at two each -- they run in rounds, and a workgroup starts on LDS that another hypothesis has filled.  The default sub_batch of
    512 would split 513 hypotheses into launches of 512 and 1; with sub_batch = 1024 one launch sees all 513 workgroups."""
    assert api.get_option("sub_batch") == 512
    poses = synth.hypotheses(n)
    try:
        api.set_option("sub_batch", 1024)
        forms_match(lambda slot: batch(slot, model, poses, frame, gscenes["proj"], crit(2)), [(8, 1, -1), (8, 0, -1)])
    finally:
        api.set_option("sub_batch", 512)


def test_the_library_chooses_for_a_full_chip(gpu, model, frame, gscenes):
    """loop_waves = 0 and loop_lds_tables = -1 with 257 hypotheses, at least one per compute unit of an MI355X (256): the library takes the
    8-wave form with the tables in LDS, says so, and the bytes are the same."""
    poses = synth.hypotheses(257)
    try:
        api.set_option("resident_loop", 0)
        batch(0, model, poses, frame, gscenes["proj"], crit(2))
        ref = batch(1, model, poses, frame, gscenes["proj"], crit(2))
        api.set_option("resident_loop", 1)
        before = resident_batches()
        assert same(batch(0, model, poses, frame, gscenes["proj"], crit(2)), ref)
        assert resident_batches() == before + 1
        assert api.get_option("stat_loop_waves") == 8 and api.get_option("stat_loop_lds_tables") == table_bytes(W, H)
    finally:
        api.set_option("resident_loop", 1)


def corner_shift(corner, K, z):
    """Translation that carries a point on the optical axis at depth z to the frame's first (0) or last (1) pixel."""
    u, v = ((0.0, 0.0), (W - 1.0, H - 1.0))[corner]
    return f32((u - K[2]) / K[0] * z), f32((v - K[5]) / K[4] * z)


def test_table_edges(gpu, model, scenario, frame):
    """Hypotheses and scene objects astride the frame's first and last pixel: their pixel boxes touch column 0 / row 0 and the last column /
    row, so the first and last entries of both tables are read and used; after the first update points leave the image and read entry 0."""
    K, proj = scenario["K"], scenario["proj"]
    base = synth.scene_pose().reshape(4, 4)
    depth = None
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    for corner in (0, 1):
        dx, dy = corner_shift(corner, K, base[2, 3])
        p = base.copy()
        p[0, 3] = dx; p[1, 3] = dy
        d = api.render_host(model, p[None], W, H, proj)[0]
        depth = d if depth is None else np.where(d > 0, d, depth)
        for q in poses[corner::2]:
            q[0, 3] += dx - base[0, 3]; q[1, 3] += dy - base[1, 3]
    assert depth[0, 0] > 0 and depth[H - 1, W - 1] > 0
    boxes = np.array([api.tight_box(scenario["tris"], q, W, H, proj)[0] for q in poses])
    # (the box's rows count from the other end of the frame than the pixel formula above: one group touches row 0, the other the last row)
    assert (boxes[0::2, 0] == 0).all() and (boxes[1::2, 2] == W - 1).all(), boxes
    assert ((boxes[0::2, 1] == 0).all() and (boxes[1::2, 3] == H - 1).all()) or ((boxes[0::2, 3] == H - 1).all() and (boxes[1::2, 1] == 0).all()), boxes
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    res, sizes = forms_match(lambda slot: batch(slot, model, poses, frame, scene, crit(2)), [(w, t, -1) for w in WAVES for t in (0, 1)])
    for group in (slice(0, None, 2), slice(1, None, 2)):            # at each corner hypotheses have points, and points that find the scene
        assert ((sizes[group] > 0) & (res["fitness"][group] > 0)).any(), (sizes, res["fitness"])


def test_another_frame(gpu, model):
    """96 x 64 with the intrinsics scaled: the table lengths come from the scene, not from 640 and 480."""
    w, h, s = 96, 64, f32(0.15)
    K = synth.K_TEST.copy()
    K[[0, 2]] *= s
    K[4] *= s
    K[5] = f32(h / 2)
    proj = api.compute_proj(K, w, h)
    depth = api.render_host(model, synth.scene_pose()[None], w, h, proj)[0]
    assert (depth > 0).sum() > 200
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K, w, h)
    small = (w, h, proj, K)
    res, sizes = forms_match(lambda slot: batch(slot, model, synth.hypotheses(8), small, scene, crit(2)),
                             [(wv, t, -1) for wv in WAVES for t in (0, 1, -1)], size=(w, h))
    assert table_bytes(w, h) == 640
    assert sizes.max() > 0 and ((sizes > 0) & (res["fitness"] > 0)).any(), (sizes, res["fitness"])
