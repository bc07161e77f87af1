"""GPU tests (-m gpu) of the library's spatially ordered copy of a triangle buffer (option mesh_order): the asynchronous path rasterises the
copy, the image is a per-pixel minimum, so every output is byte-identical with and without it; and the copy is an assumption about memory the
caller owns, re-verified by every batch -- box and multiset fingerprint of the caller's buffer -- so a buffer rewritten behind the library's
back costs one repeated batch (api.stats()[0]) and never a wrong one."""

import numpy as np
import pytest

from pose_refine_amd import api, synth
from gpu_common import W, H, raw_h2d

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0, 0)


def through_slots(m, poses, scenario, scene, crit, roi=NONE):
    """The batch on slot 0 and its reverse on slot 1, both in flight together; returns ((records, sizes), (records, sizes))."""
    api.refine_submit(0, m, poses, W, H, scenario["proj"], scenario["K"], scene, crit, roi=roi)
    api.refine_submit(1, m, poses[::-1].copy(), W, H, scenario["proj"], scenario["K"], scene, crit, roi=roi)
    return api.refine_wait(0), api.refine_wait(1)


def synchronous(m, poses, scenario, scene, crit, roi=NONE):
    """The synchronous path (a timed call never goes through a slot): everything derived on the device from the caller's buffer, per call."""
    api.set_option("profile", 1)
    try:
        return api.refine_batch(m, poses, W, H, scenario["proj"], scenario["K"], scene, crit, roi=(roi if roi != NONE else None))
    finally:
        api.set_option("profile", 0)


def both_orders_match_the_synchronous_call(m, poses, scenario, scene, crit, roi=NONE):
    ref, ref_sizes = synchronous(m, poses, scenario, scene, crit, roi)
    assert ref_sizes.max() > 0
    try:
        for order in (0, 1, 0, 1):                                   # (switching back and forth: a copy made once is found again)
            api.set_option("mesh_order", order)
            (a, sa), (b, sb) = through_slots(m, poses, scenario, scene, crit, roi)
            assert np.array_equal(sa, ref_sizes) and a.tobytes() == ref.tobytes(), f"mesh_order={order}, slot 0"
            assert np.array_equal(sb, ref_sizes[::-1]) and b.tobytes() == ref[::-1].tobytes(), f"mesh_order={order}, slot 1"
    finally:
        api.set_option("mesh_order", 1)


@pytest.mark.device_solve
def test_headline_batch_is_byte_identical_in_either_order(gpu, model, scenario, gscenes):
    """BASELINE configs[1]: obj_06, 256 hypotheses, projective scene, 20 iterations."""
    repeated = api.stats()[0]
    both_orders_match_the_synchronous_call(model, synth.hypotheses(256), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 20))
    assert api.stats()[0] == repeated


@pytest.mark.device_solve
def test_roi_batch_is_byte_identical_in_either_order(gpu, model, scenario, gscenes):
    both_orders_match_the_synchronous_call(model, synth.hypotheses(96), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 8), roi=(250, 150, 180, 160))


@pytest.mark.device_solve
def test_kdtree_scene_batch_is_byte_identical_in_either_order(gpu, model, scenario, gscenes):
    both_orders_match_the_synchronous_call(model, synth.hypotheses(64), scenario, gscenes["nn"], api.ICPConvergenceCriteria(0.0, 0.0, 6))


def test_host_solve_batch_is_byte_identical_in_either_order(gpu, model, scenario, gscenes):
    """Host solve: the slots' helper threads run the synchronous path in private contexts (no copy there; nothing may change)."""
    both_orders_match_the_synchronous_call(model, synth.hypotheses(64), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 6))


@pytest.mark.device_solve
def test_streamed_mesh_is_byte_identical_in_either_order(gpu, scenario, gscenes):
    """A uv-sphere of 90 000 triangles (3.24 MB: beyond the 3 MiB up to which a raster workgroup takes one hypothesis, so each walks a run
    of hypotheses with its triangles), in grid order in the caller's buffer."""
    tris = synth.uv_sphere_mesh(300, 150)
    assert tris.nbytes > (3 << 20)
    both_orders_match_the_synchronous_call(api.Model(tris=tris), synth.hypotheses(48), scenario, gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 4))


def box_of(tris):
    v = tris.reshape(-1, 3)
    return v.min(0), v.max(0)


def interior_vertices_moved(tris):
    """The same triangles with the vertices of every seventh triangle pulled a fifth of the way towards the middle of the box -- except
    vertices that lie on the box: it stays, bit for bit."""
    lo, hi = box_of(tris)
    out = tris.copy()
    mid = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    sel = out[::7]
    on_box = np.any((sel == lo) | (sel == hi), axis=-1, keepdims=True)
    out[::7] = np.where(on_box, sel, (sel + (mid - sel) * np.float32(0.2)).astype(np.float32))
    return out


def scaled_into_box(tris, lo, hi):
    """Another mesh mapped axis by axis into the box [lo, hi], its extreme vertices exactly on it."""
    a, b = box_of(tris)
    out = ((tris - a) / (b - a) * (hi - lo) + lo).astype(np.float32)
    out = np.clip(out, lo, hi)
    flat_in, flat_out = tris.reshape(-1, 3), out.reshape(-1, 3)
    for d in range(3):
        flat_out[flat_in[:, d] == a[d], d] = lo[d]
        flat_out[flat_in[:, d] == b[d], d] = hi[d]
    return np.ascontiguousarray(out)


@pytest.mark.device_solve
@pytest.mark.parametrize("case", ["interior_vertices_moved", "another_mesh_in_the_same_box"])
def test_buffer_rewritten_with_the_same_box_is_never_rendered_from_the_stale_copy(gpu, scenario, gscenes, case):
    first = scenario["tris"][:20000].copy()
    lo, hi = box_of(first)
    second = interior_vertices_moved(first) if case == "interior_vertices_moved" else scaled_into_box(scenario["tris"][11468:31468].copy(), lo, hi)
    assert second.shape == first.shape and not np.array_equal(second, first)
    assert np.array_equal(box_of(second)[0], lo) and np.array_equal(box_of(second)[1], hi)      # the box check alone cannot see this rewrite
    poses = synth.hypotheses(40)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 4)
    args = (W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    m = api.Model(tris=first)
    ref = {}
    for name, content in (("first", first), ("second", second)):
        ref[name] = synchronous(api.Model(tris=content), poses, scenario, gscenes["proj"], crit)
    assert ref["first"][0].tobytes() != ref["second"][0].tobytes() or not np.array_equal(ref["first"][1], ref["second"][1])

    def slot_batch(slot, expect):
        api.refine_submit(slot, m, poses, *args)
        r, s = api.refine_wait(slot)
        assert np.array_equal(s, ref[expect][1]) and r.tobytes() == ref[expect][0].tobytes()

    slot_batch(0, "first")
    slot_batch(1, "first")                                           # box and ordered copy of `first` are cached now (the copy from the second batch on)
    repeated = api.stats()[0]
    for k, (name, content) in enumerate((("second", second), ("first", first), ("second", second))):
        raw_h2d(m.device_tris().data(), content)                     # behind the library's back: same address, same count, same box
        # synchronously: nothing is cached, nothing is repeated
        r, s = synchronous(m, poses, scenario, gscenes["proj"], crit)
        assert np.array_equal(s, ref[name][1]) and r.tobytes() == ref[name][0].tobytes()
        assert api.stats()[0] == repeated + k
        # through the slots: the first batch after the rewrite is repeated, and only that one
        slot_batch(k & 1, name)
        assert api.stats()[0] == repeated + k + 1
        slot_batch(1 - (k & 1), name)
        (a, sa), (b, sb) = through_slots(m, poses, scenario, gscenes["proj"], crit)
        assert np.array_equal(sa, ref[name][1]) and a.tobytes() == ref[name][0].tobytes()
        assert np.array_equal(sb, ref[name][1][::-1]) and b.tobytes() == ref[name][0][::-1].tobytes()
        assert api.stats()[0] == repeated + k + 1
    # the caller's triangles permuted in place: the same multiset, the same image -- not flagged
    repeated = api.stats()[0]
    raw_h2d(m.device_tris().data(), np.ascontiguousarray(second[np.random.default_rng(4).permutation(len(second))]))
    slot_batch(0, "second")
    slot_batch(1, "second")
    assert api.stats()[0] == repeated


@pytest.mark.device_solve
def test_fifty_pipelined_steps_repeat_nothing(gpu, model, scenario, gscenes):
    """The benchmark's loop: step k is submitted on slot k & 1, then step k - 1 is waited for.  The per-batch check raises no false alarm."""
    poses = synth.hypotheses(256)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    ref, ref_sizes = synchronous(model, poses, scenario, gscenes["proj"], crit)
    for _ in range(2):                                               # (the box on the buffer's first batch, the ordered copy on its second: once)
        api.refine_submit(0, model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        api.refine_wait(0)
    repeated = api.stats()[0]
    inflight = [False, False]
    for k in range(50):
        b = k & 1
        api.refine_submit(b, model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        inflight[b] = True
        if inflight[1 - b]:
            r, s = api.refine_wait(1 - b)
            inflight[1 - b] = False
            assert np.array_equal(s, ref_sizes) and r.tobytes() == ref.tobytes()
    for b in (0, 1):
        if inflight[b]:
            r, s = api.refine_wait(b)
            assert np.array_equal(s, ref_sizes) and r.tobytes() == ref.tobytes()
    assert api.stats()[0] == repeated
