"""GPU tests (-m gpu) of the asynchronous path's tight pixel boxes (option tight_box): each hypothesis' box comes from the mesh's projected
vertices (pose_tight_box_kernel over the library's list of the buffer's distinct vertices) instead of the projected corners of its box.  A
box that holds every pixel the raster can draw changes no output: every batch must be byte-identical with the option off and on -- T,
fitness, rmse and cloud sizes.  The list is an assumption about memory the caller owns, verified with the ordered copy by every batch: a
buffer rewritten behind the library's back must never be clipped by a stale list.  Read-only option stat_tight_batches counts the batches
that really ran on tight boxes, so that no case passes by quietly staying on the loose ones."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H, raw_h2d

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0, 0)
f32 = np.float32


def batch(slot, m, poses, scenario, scene, crit, roi=NONE):
    api.refine_submit(slot, m, poses, W, H, scenario["proj"], scenario["K"], scene, crit, roi=roi)
    return api.refine_wait(slot)


def same(a, b):
    return np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()


def tight_batches():
    return api.get_option("stat_tight_batches")


def loose_and_tight_match(m, poses, scenario, scene, crit, roi=NONE, expect_tight=2):
    """Reference with tight_box = 0 (two batches first: the vertex list is made on a buffer's second batch), then one batch per slot with
    tight_box = 1.  Returns the reference."""
    try:
        api.set_option("tight_box", 0)
        before = tight_batches()
        batch(0, m, poses, scenario, scene, crit, roi)
        ref = batch(1, m, poses, scenario, scene, crit, roi)
        assert tight_batches() == before
        api.set_option("tight_box", 1)
        for slot in (0, 1):
            assert same(batch(slot, m, poses, scenario, scene, crit, roi), ref), f"tight_box=1, slot {slot}"
        assert tight_batches() == before + expect_tight
        api.set_option("tight_box", 0)
        assert same(batch(0, m, poses, scenario, scene, crit, roi), ref)
    finally:
        api.set_option("tight_box", 1)
    return ref


CRIT = api.ICPConvergenceCriteria(0.0, 0.0, 6)


@pytest.mark.device_solve
def test_projective_scene(gpu, model, scenario, gscenes):
    ref = loose_and_tight_match(model, synth.hypotheses(8), scenario, gscenes["proj"], CRIT)
    assert ref[1].min() > 0


@pytest.mark.device_solve
def test_kdtree_scene(gpu, model, scenario, gscenes):
    ref = loose_and_tight_match(model, synth.hypotheses(8), scenario, gscenes["nn"], CRIT)
    assert ref[1].min() > 0


def test_host_solve_stays_on_the_synchronous_path(gpu, model, scenario, gscenes):
    """Host solve: the slots' helper threads run the synchronous path, which keeps its boxes -- nothing may change, no batch counts as tight."""
    loose_and_tight_match(model, synth.hypotheses(8), scenario, gscenes["proj"], CRIT, expect_tight=0)


@pytest.mark.device_solve
def test_roi(gpu, model, scenario, gscenes):
    ref = loose_and_tight_match(model, synth.hypotheses(8), scenario, gscenes["proj"], CRIT, roi=(250, 150, 180, 160))
    assert ref[1].max() > 0


@pytest.mark.device_solve
@pytest.mark.parametrize("n", [1, 257])                            # 257: the offset scan carries over its 256-entry chunk
def test_batch_sizes(gpu, model, scenario, gscenes, n):
    loose_and_tight_match(model, synth.hypotheses(n), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 2))


@pytest.mark.device_solve
def test_offsets_restart_at_every_sub_batch(gpu, model, scenario, gscenes):
    try:
        api.set_option("sub_batch", 32)
        loose_and_tight_match(model, synth.hypotheses(40), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 2))
    finally:
        api.set_option("sub_batch", 512)


def near_plane_pose(tris, pose):
    """The pose pushed towards the camera until the nearest vertex stands 0.5 micrometres in front of the camera plane (z <= 1e-3)."""
    p = pose.copy().reshape(4, 4)
    v = np.unique(tris.reshape(-1, 3), axis=0)
    lz = p[2, 0] * v[:, 0] + p[2, 1] * v[:, 1] + p[2, 2] * v[:, 2]
    p[2, 3] = f32(5e-4) - lz.min()
    return p


@pytest.mark.device_solve
def test_special_poses(gpu, model, scenario, gscenes):
    """Half out of the frame; wholly outside (empty box, empty cloud, identity result); a vertex at the camera plane (the loose box stays)."""
    tris = scenario["tris"]
    poses = synth.hypotheses(8).copy().reshape(-1, 4, 4)
    poses[1, 0, 3] += f32(150.0)
    poses[3, 0, 3] += f32(2000.0)
    poses[5] = near_plane_pose(tris, poses[5])
    tight, loose = zip(*(api.tight_box(tris, poses[i], W, H, scenario["proj"]) for i in (1, 3, 5)))
    assert tight[0][2] == W - 1 and tight[0][0] > 0
    assert tight[1][2] < tight[1][0]
    assert np.array_equal(tight[2], loose[2]) and np.array_equal(loose[2], [0, 0, W - 1, H - 1])
    res, sizes = loose_and_tight_match(model, poses, scenario, gscenes["proj"], CRIT)
    assert sizes[3] == 0 and np.array_equal(res["T"][3].reshape(4, 4), np.eye(4, dtype=f32))
    assert sizes[1] > 0 and sizes[5] > 0


def cube(size):
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32) * f32(size)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.ascontiguousarray([[c[q[0]], c[q[1]], c[q[2]]] for q in quads] + [[c[q[0]], c[q[2]], c[q[3]]] for q in quads], f32)


@pytest.mark.device_solve
@pytest.mark.parametrize("mesh", ["one_triangle", "cube"])
def test_tiny_meshes(gpu, scenario, gscenes, mesh):
    tris = np.array([[[-40, -30, 0], [45, -20, 5], [0, 50, -5]]], f32) if mesh == "one_triangle" else cube(35.0)
    ref = loose_and_tight_match(api.Model(tris=tris), synth.hypotheses(8), scenario, gscenes["proj"], CRIT)
    assert ref[1].min() > 0


@pytest.mark.device_solve
def test_first_batch_of_a_fresh_context_is_loose_the_second_tight(gpu, model, scenario, gscenes):
    poses = synth.hypotheses(8)
    try:
        api.set_option("tight_box", 0)
        ref = batch(0, model, poses, scenario, gscenes["proj"], CRIT)
        api.shutdown(); api.init(0); api.set_option("solve", api.SOLVE_DEVICE)
        api.set_option("tight_box", 1)
        before = tight_batches()
        assert same(batch(0, model, poses, scenario, gscenes["proj"], CRIT), ref)
        assert tight_batches() == before                            # no list yet: the loose path
        assert same(batch(1, model, poses, scenario, gscenes["proj"], CRIT), ref)
        assert tight_batches() == before + 1
    finally:
        api.set_option("tight_box", 1)


@pytest.mark.device_solve
def test_buffer_rewritten_in_place_is_never_clipped_by_the_stale_list(gpu, scenario, gscenes):
    first = scenario["tris"][:20000].copy()
    v = first.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    second = first.copy()
    second[777, 1] = (lo + (hi - lo) * f32(0.97)).astype(f32)       # one vertex out to near a corner of the box: inside it, far outside the surface
    assert np.array_equal(second.reshape(-1, 3).min(0), lo) and np.array_equal(second.reshape(-1, 3).max(0), hi)
    poses = synth.hypotheses(8)
    grown = [api.tight_box(second, p, W, H, scenario["proj"])[0] for p in poses]
    stale = [api.tight_box(first, p, W, H, scenario["proj"])[0] for p in poses]
    assert any(g[0] < s[0] or g[1] < s[1] or g[2] > s[2] or g[3] > s[3] for g, s in zip(grown, stale))     # the stale boxes WOULD clip
    m = api.Model(tris=first)
    ref = {}
    api.set_option("profile", 1)                                    # the synchronous path: everything from the caller's buffer, per call
    try:
        for name, content in (("first", first), ("second", second)):
            ref[name] = api.refine_batch(api.Model(tris=content), poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    finally:
        api.set_option("profile", 0)
    assert not same(ref["first"], ref["second"])
    before = tight_batches()
    for slot in (0, 1, 0):
        assert same(batch(slot, m, poses, scenario, gscenes["proj"], CRIT), ref["first"])
    assert tight_batches() == before + 2
    repeated = api.stats()[0]
    raw_h2d(m.device_tris().data(), second)                         # behind the library's back: same address, same count, same box
    assert same(batch(1, m, poses, scenario, gscenes["proj"], CRIT), ref["second"])
    assert api.stats()[0] == repeated + 1                           # flagged by the fingerprint, run again from the caller's buffer
    for slot in (0, 1, 0):                                          # the box again, then the new list: tight on the new content
        assert same(batch(slot, m, poses, scenario, gscenes["proj"], CRIT), ref["second"])
    assert api.stats()[0] == repeated + 1


@pytest.mark.device_solve
def test_twenty_pipelined_steps_repeat_the_same_bytes(gpu, model, scenario, gscenes):
    poses = synth.hypotheses(64)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 8)
    ref = loose_and_tight_match(model, poses, scenario, gscenes["proj"], crit)
    before, repeated = tight_batches(), api.stats()[0]
    inflight = [False, False]
    for k in range(20):
        b = k & 1
        api.refine_submit(b, model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        inflight[b] = True
        if inflight[1 - b]:
            assert same(api.refine_wait(1 - b), ref)
            inflight[1 - b] = False
    for b in (0, 1):
        if inflight[b]:
            assert same(api.refine_wait(b), ref)
    assert tight_batches() == before + 20 and api.stats()[0] == repeated
