"""GPU tests (-m gpu) of caches keyed by caller-owned addresses (model box, packed scene, kd-tree records): write log, device-side checks, sampled fingerprint.
The HIP path is called through the C ABI (pose_refine_amd.api) and held to the CPU oracle on the same inputs: integers, inlier counts and
per-pass sums bit-exact, transforms within 1e-4 (north_star).  @pytest.mark.device_solve = the 6x6 solve runs on the device (the headline
configuration); without it the solve is on the host, as icp.cu:207 does it."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import *  # noqa: F401,F403 -- W, H, TOL_T, inliers, raw_h2d, make_scene, random_mesh ...

pytestmark = pytest.mark.gpu


# ---- caches keyed by the caller's addresses -----------------------------------------------------------------------------
@pytest.mark.device_solve
def test_rewritten_triangle_buffer_is_never_rendered_with_a_stale_box(gpu, scenario, gscenes):
    """the asynchronous path sizes a batch from a host copy of the model box keyed by (pointer, size).
    The buffer is rewritten here behind the library's back (raw hipMemcpy, same address, same triangle count) with a mesh
    twice the size: the batch must come out as if the box had been recomputed."""
    tris = scenario["tris"][:20000].copy()
    big = (tris * np.float32(1.6)).astype(np.float32)
    poses = synth.hypotheses(40)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 4)
    m = api.Model(tris=tris)
    r0, s0 = api.refine_batch(m, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)      # caches the small box
    ref_big, ref_sizes = api.refine_batch(api.Model(tris=big), poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    raw_h2d(m.device_tris().data(), big)
    r1, s1 = api.refine_batch(m, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    assert np.array_equal(s1, ref_sizes) and r1.tobytes() == ref_big.tobytes()
    assert not np.array_equal(s0, s1)
    # and through the two asynchronous slots, with the stale box detected at wait time
    raw_h2d(m.device_tris().data(), tris)
    api.refine_submit(0, m, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    api.refine_submit(1, m, poses[::-1].copy(), W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    a, sa = api.refine_wait(0)
    b, sb = api.refine_wait(1)
    assert np.array_equal(sa, s0) and a.tobytes() == r0.tobytes()
    assert np.array_equal(sb, s0[::-1]) and b.tobytes() == r0[::-1].tobytes()


@pytest.mark.device_solve
def test_scene_cache_follows_writes(gpu, model, scenario):
    """The packed projective scene is cached by the address of the caller's arrays: writes through the library drop it,
    writes the library cannot see need pr_invalidate (documented contract), scene_cache=0 never caches."""
    K = scenario["K"]
    d1, d0 = scenario["depth"][1], scenario["depth"][0]
    poses = synth.hypotheses(8)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 5)
    sa = api.Scene_projective().init_Scene_projective_cuda(d1, K)
    sb = api.Scene_projective().init_Scene_projective_cuda(d0, K)
    ra, _ = api.refine_batch(model, poses, W, H, scenario["proj"], K, sa, crit)
    rb, _ = api.refine_batch(model, poses, W, H, scenario["proj"], K, sb, crit)
    assert ra.tobytes() != rb.tobytes()
    lib = _lib.load()
    # (1) overwrite scene A's arrays with scene B's content through the library: the cache must notice
    n = sa.pcd_buffer.size() * 4
    api.check(lib.pr_memcpy_d2d(sa.pcd_buffer.data(), sb.pcd_buffer.data(), n))
    api.check(lib.pr_memcpy_d2d(sa.normal_buffer.data(), sb.normal_buffer.data(), n))
    r1, _ = api.refine_batch(model, poses, W, H, scenario["proj"], K, sa, crit)
    assert r1.tobytes() == rb.tobytes()
    # (2) back to scene A behind the library's back + pr_invalidate
    sa2 = api.Scene_projective().init_Scene_projective_cuda(d1, K)
    raw_h2d(sa.pcd_buffer.data(), sa2.pcd_host)
    raw_h2d(sa.normal_buffer.data(), sa2.normal_host)
    api.invalidate(sa.pcd_buffer.data(), n)
    api.invalidate(sa.normal_buffer.data())                      # 0 bytes = the whole allocation
    r2, _ = api.refine_batch(model, poses, W, H, scenario["proj"], K, sa, crit)
    assert r2.tobytes() == ra.tobytes()
    # (3) caches off: raw writes are picked up without any announcement
    api.set_option("scene_cache", 0)
    try:
        raw_h2d(sa.pcd_buffer.data(), sb.pcd_host)
        raw_h2d(sa.normal_buffer.data(), sb.normal_host)
        r3, _ = api.refine_batch(model, poses, W, H, scenario["proj"], K, sa, crit)
        assert r3.tobytes() == rb.tobytes()
    finally:
        api.set_option("scene_cache", 1)


@pytest.mark.device_solve
def test_scene_rewritten_behind_the_librarys_back_is_noticed(gpu, model, scenario):
    """the packed projective scene (like the kd-tree search records) is cached by the address of the caller's arrays.  A frame
    that is replaced as a whole through a raw hipMemcpy (no pr_invalidate) changes the sampled fingerprint every asynchronous batch takes
    of those arrays: the batch is repeated with fresh caches and returns what a new scene object returns.  (A kd-tree scene of another
    frame has other point and node counts, which are part of its cache key.)"""
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 6)
    poses = synth.hypotheses(48)
    K = scenario["K"]
    a = api.Scene_projective().init_Scene_projective_cuda(scenario["depth"][1], K)
    b = api.Scene_projective().init_Scene_projective_cuda(scenario["depth"][0], K)       # another frame of the same size
    want_b = api.refine_batch(model, poses, W, H, scenario["proj"], K, b, crit)
    first = api.refine_batch(model, poses, W, H, scenario["proj"], K, a, crit)      # the caches of `a` are built here
    assert first[0].tobytes() != want_b[0].tobytes()
    raw_d2d(a.normal_buffer.data(), b.normal_buffer.data(), a.normal_buffer.size() * 4)
    raw_d2d(a.pcd_buffer.data(), b.pcd_buffer.data(), a.pcd_buffer.size() * 4)
    repeated0 = api.stats()[0]
    got = api.refine_batch(model, poses, W, H, scenario["proj"], K, a, crit)
    assert got[0].tobytes() == want_b[0].tobytes() and np.array_equal(got[1], want_b[1])
    assert api.stats()[0] == repeated0 + 1                      # the repeated batch is counted (pr_stats), not silent
    got = api.refine_batch(model, poses, W, H, scenario["proj"], K, a, crit)
    assert got[0].tobytes() == want_b[0].tobytes() and api.stats()[0] == repeated0 + 1      # fresh caches: nothing to repeat


@pytest.mark.device_solve
def test_kdtree_scene_rewritten_behind_the_librarys_back_is_noticed_by_a_bare_icp_call(gpu, scenario):
    """The same for the kd-tree search records and a synchronous call (pr_icp_nn checks a cache hit on the spot): points and nodes of a
    scene are replaced by those of a shifted copy with the same counts, through raw copies."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-0.1, 0.1, size=(5000, 3)).astype(np.float32)
    nrm = rng.normal(size=(5000, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = make_scene(pts.copy(), nrm.copy(), 10)
    b = make_scene((pts + np.float32(0.003)).astype(np.float32), nrm.copy(), 10)
    if len(a.nodes_host) != len(b.nodes_host):
        pytest.skip("the shifted copy built a tree of another size")
    cloud = rng.uniform(-0.1, 0.1, size=(3000, 3)).astype(np.float32)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 5)
    run = lambda sc: api.ICP_Point2Plane(api.DeviceVector.from_host(cloud.reshape(-1)), sc, crit)
    want_b, first = run(b), run(a)                                # the search records of `b`, then of `a`, are built here
    assert not np.array_equal(first.transformation_, want_b.transformation_)
    for dst, src in ((a.pcd_buffer, b.pcd_buffer), (a.normal_buffer, b.normal_buffer)):
        raw_d2d(dst.data(), src.data(), dst.size() * 4)
    raw_d2d(a.nodes.data(), b.nodes.data(), len(a.nodes_host) * 52)
    got = run(a)
    assert np.array_equal(got.transformation_, want_b.transformation_) and got.fitness_ == want_b.fitness_


@pytest.mark.device_solve
def test_kdtree_scenes_that_change_every_frame_keep_both_slots_running(gpu, model, scenario):
    """a NEW kd-tree scene per frame, frames pipelined through the two slots.  The library keeps two sets of derived records
    (pr_runtime.h NNDerived): the set a batch in flight reads is never rebuilt under it -- three scenes in rotation (every frame finds neither set
    holding its scene while the other slot still reads one of them), then ONE scene object re-initialised on the device frame after frame while the
    previous frame's batch runs on a second object.  Every frame's records equal the synchronous call's against the same scene (which
    test_golden_full_gpu / test_kdtree_search_gpu hold to the oracle), bit for bit."""
    K, proj = scenario["K"], scenario["proj"]
    poses = synth.hypotheses(48)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 6)
    base = scenario["depth"][1].astype(np.int32)
    depths = []
    for i in range(3):
        d = base.copy()
        d[d > 0] += 3 * i                                            # the same surface 0 / 3 / 6 mm further away: different trees, different answers
        d[(40 * i) % H::7, ::5] = 0
        depths.append(d)
    scenes = [api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(d.reshape(-1)), K, W, H) for d in depths]
    want = [api.refine_batch(model, poses, W, H, proj, K, s, crit) for s in scenes]
    assert want[0][0].tobytes() != want[1][0].tobytes() != want[2][0].tobytes()
    repeated_before = api.stats()[0]
    # (1) three scenes in rotation over two slots
    for k in range(9):
        api.refine_submit(k & 1, model, poses, W, H, proj, K, scenes[k % 3], crit)
        if k:
            res, sizes = api.refine_wait((k - 1) & 1)
            assert res.tobytes() == want[(k - 1) % 3][0].tobytes() and np.array_equal(sizes, want[(k - 1) % 3][1])
    res, sizes = api.refine_wait(0)
    assert res.tobytes() == want[8 % 3][0].tobytes()
    # (2) two scene objects re-initialised in turn from images on the device, each while the other one's batch is in flight
    devs = [api.DeviceVector.from_host(d.reshape(-1)) for d in depths]
    objs = [api.Scene_nn(), api.Scene_nn()]
    for k in range(8):
        objs[k & 1].init_Scene_nn_device(devs[k % 3], K, W, H)      # (slot k & 1 delivered its previous batch two frames ago: its scene object is free)
        api.refine_submit(k & 1, model, poses, W, H, proj, K, objs[k & 1], crit)
        if k:
            res, sizes = api.refine_wait((k - 1) & 1)
            assert res.tobytes() == want[(k - 1) % 3][0].tobytes() and np.array_equal(sizes, want[(k - 1) % 3][1])
    res, _ = api.refine_wait(1)
    assert res.tobytes() == want[7 % 3][0].tobytes()
    assert api.stats()[0] == repeated_before                        # (no batch had to be run again by the stale-cache safety net)


@pytest.mark.device_solve
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_one_scene_object_reinitialised_under_its_own_batch_in_flight(gpu, model, scenario, kind):
    """a scene object keeps its arrays across re-initialisation, so `submit k; init scene k+1 on the SAME object; wait k` has the
    preparation of frame k+1 write the arrays batch k is still reading.  The library orders such a write behind the batches of the context that
    read the range (drain_slots_reading, pr_runtime.h) -- the reference reads the caller's arrays at every call (depth_scene.h:29-48) and its
    uploads are synchronous, so a caller written against it may do exactly this.  Every frame's records equal the synchronous call's."""
    K, proj = scenario["K"], scenario["proj"]
    poses = synth.hypotheses(64)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 8)
    base = scenario["depth"][1].astype(np.int32)
    depths = []
    for i in range(3):
        d = base.copy()
        d[d > 0] += 4 * i
        d[(30 * i) % H::9, ::4] = 0
        depths.append(d)
    devs = [api.DeviceVector.from_host(d.reshape(-1)) for d in depths]
    make = (lambda s, dv: s.init_Scene_projective_device(dv, K, W, H)) if kind == "proj" else (lambda s, dv: s.init_Scene_nn_device(dv, K, W, H))
    want = [api.refine_batch(model, poses, W, H, proj, K, make(api.Scene_projective() if kind == "proj" else api.Scene_nn(), dv), crit) for dv in devs]
    assert want[0][0].tobytes() != want[1][0].tobytes() != want[2][0].tobytes()
    one = api.Scene_projective() if kind == "proj" else api.Scene_nn()
    make(one, devs[0])
    for k in range(7):
        api.refine_submit(k & 1, model, poses, W, H, proj, K, one, crit)
        make(one, devs[(k + 1) % 3])                                 # the next frame's scene into the SAME arrays, batch k in flight
        if k:
            res, sizes = api.refine_wait((k - 1) & 1)
            assert res.tobytes() == want[(k - 1) % 3][0].tobytes() and np.array_equal(sizes, want[(k - 1) % 3][1]), k
    res, _ = api.refine_wait(0)
    assert res.tobytes() == want[6 % 3][0].tobytes()


FRAME_STAGES = ["depth_fuse", "depth_filter", "depth_reproject", "scene_planes", "segment_depth"]


@pytest.mark.device_solve
@pytest.mark.parametrize("stage", FRAME_STAGES)
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_frame_stage_output_over_a_scene_of_a_batch_in_flight(gpu, model, scenario, kind, stage):
    """The frame stages' outputs are ordered like every other write through the library (note_write, pr_runtime.h): a stage whose ``depth_out`` lies
    over the point array of the scene a pending batch reads waits for that batch, then writes.  The batch returns the synchronous call's bytes, the
    range holds what the same stage call writes into a buffer of its own, and no batch is repeated.  (Before the stages announced their writes
    ahead of their launches this was a race; a pass of a race proves nothing, so the order of note_write and the launches is also a matter of
    reading csrc/pr_*.cpp.)"""
    K, proj = scenario["K"], scenario["proj"]
    poses = synth.hypotheses(64)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 8)
    base = scenario["depth"][1].astype(np.int32)
    later = base.copy()
    later[later > 0] += 4
    d_a, d_b = api.DeviceVector.from_host(base.reshape(-1)), api.DeviceVector.from_host(later.reshape(-1))
    fresh = (lambda: api.Scene_projective().init_Scene_projective_device(d_a, K, W, H)) if kind == "proj" else (lambda: api.Scene_nn().init_Scene_nn_device(d_a, K, W, H))
    S = fresh()
    want = api.refine_batch(model, poses, W, H, proj, K, S, crit)
    other = api.Scene_projective().init_Scene_projective_device(d_b, K, W, H)      # scene_planes' own scene: another object
    labels = api.scene_segments(d_a, W, H, min_pixels=16)[1]
    run = {
        "depth_fuse": lambda out: api.depth_fuse([d_a, d_b], W, H, depth_out=out),
        "depth_filter": lambda out: api.depth_filter(d_b, W, H, depth_out=out, radius=1, fill_min=5)[0],
        "depth_reproject": lambda out: api.depth_reproject([api.ReprojectSource.frame(d_b, W, H, K)], W, H, K, dtype=np.int32, depth_out=out)[0],
        "scene_planes": lambda out: api.scene_planes(other, d_b, depth_out=out, min_support=50)[2],
        "segment_depth": lambda out: api.segment_depth(labels, d_a, [1], depth_out=out),
    }[stage]
    own = run(None).to_host()                                       # what the stage writes into a buffer of its own
    assert own.dtype == np.int32 and own.size == W * H and own.any()
    over = api.DeviceVector(W * H, np.int32, _adopt=S.pcd_buffer.data())      # the first W * H words of the scene's point array
    repeated = api.stats()[0]
    try:
        api.refine_submit(0, model, poses, W, H, proj, K, S, crit)
        run(over)                                                   # batch 0 in flight
        res, sizes = api.refine_wait(0)
        got = over.to_host()
    finally:
        over._ptr, over.count = None, 0                             # detached: the scene object frees its array itself
    assert res.tobytes() == want[0].tobytes() and np.array_equal(sizes, want[1])
    assert got.tobytes() == own.tobytes()
    assert api.stats()[0] == repeated


@pytest.mark.device_solve
def test_unchanged_cropped_scene_is_never_found_stale(gpu, model, scenario, gscenes):
    """Every asynchronous batch compares the sampled fingerprint of the scene arrays with the word kept behind the packed cache's tables
    (ProjTail, pr_runtime.h), over the same list of arrays in the same order as the build.  A list in another order, or a tail word at
    another offset, would flag every batch and run it twice: three batches on an unchanged cropped scene repeat nothing and return the same bytes.
    (A whole-frame projective scene: test_scene_rewritten_behind_the_librarys_back_is_noticed's last batch; kd-tree scenes:
    test_kdtree_scenes_that_change_every_frame_keep_both_slots_running.)  The window's width + height is odd: the tail sits behind padding."""
    K, proj = scenario["K"], scenario["proj"]
    ys, xs = np.nonzero(scenario["depth"][1])
    w, h = int(xs.max() - xs.min() + 1) | 1, (int(ys.max() - ys.min() + 1) + 1) & ~1      # odd, even
    x0, y0 = min(int(xs.min()), W - w), min(int(ys.min()), H - h)
    scene = gscenes["proj"].crop((x0, y0, w, h))
    poses = synth.hypotheses(8)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 4)
    repeated = api.stats()[0]
    got = []
    for k in range(3):
        api.refine_submit(k & 1, model, poses, W, H, proj, K, scene, crit)
        if k:
            got.append(api.refine_wait((k - 1) & 1))
    got.append(api.refine_wait(0))
    assert api.stats()[0] == repeated
    assert (w + h) % 4 != 0 and got[0][0]["fitness"].max() > 0.0
    for res, sizes in got[1:]:
        assert res.tobytes() == got[0][0].tobytes() and np.array_equal(sizes, got[0][1])


def sampled_words(n_words):
    """The word positions fingerprint_lane (csrc/pr_device.h) looks at in an array of n_words 32-bit words: one per stripe of n / 4096."""
    stripe = n_words // 4096
    assert stripe > 0
    s = np.arange(4096, dtype=np.uint64)
    h = (s * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    return (s * np.uint64(stripe) + ((h * np.uint64(stripe)) >> np.uint64(32))).astype(np.int64)


@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_in_place_edit_that_the_sampled_fingerprint_cannot_see_is_noticed_by_a_synchronous_call(gpu, model, scenario, solve):
    """the reference reads the caller's scene arrays at every call (depth_scene.h:29-48), and its device_vector_holder hands out
    raw mutable pointers.  Here a scene's arrays are rewritten in place through raw copies (no pr_invalidate) with another frame's content in EVERY
    word EXCEPT the 4096 the sampled fingerprint reads (those keep the old frame's values): the synchronous entry points -- what the C++ adapters
    call -- compare a fingerprint of every word and must answer like the oracle on the edited arrays.  (The edited pcd is no longer what dep2pcd
    produces for its depth, so this is also the route on which the caller's arrays are used as they are.)"""
    K = scenario["K"]
    api.set_option("solve", solve)
    try:
        a = api.Scene_projective().init_Scene_projective_cuda(scenario["depth"][1], K)
        oa, ob = O.ProjScene(scenario["depth"][1], K), O.ProjScene(scenario["depth"][0], K)
        cloud = scenario["cloud"]
        crit = (0.0, 0.0, 8)
        run = lambda: api.ICP_Point2Plane(api.DeviceVector.from_host(cloud.reshape(-1)), a, api.ICPConvergenceCriteria(*crit))
        first = run()                                                  # builds the packed copy + both fingerprints
        ref_a, _, _, _ = O.icp(cloud, oa, crit, O.SUM_CANONICAL, api.get_option("points_per_block"))
        assert first.fitness_ == float(ref_a["fitness"])
        keep = sampled_words(W * H * 3)
        for arr_b, arr_a, dev in ((ob.pcd, oa.pcd, a.pcd_buffer), (ob.normal, oa.normal, a.normal_buffer)):
            mixed = arr_b.reshape(-1).copy().view(np.uint32)
            mixed[keep] = arr_a.reshape(-1).view(np.uint32)[keep]
            raw_h2d(dev.data(), mixed)                                 # behind the library's back
            arr_b.reshape(-1).view(np.uint32)[:] = mixed               # the oracle's scene `ob` now holds exactly the edited arrays
        got = run()
        ref, _, _, _ = O.icp(cloud, ob, crit, O.SUM_CANONICAL, api.get_option("points_per_block"))
        assert float(ref["fitness"]) != float(ref_a["fitness"])
        assert got.fitness_ == float(ref["fitness"])
        assert got.inlier_rmse_ == pytest.approx(float(ref["inlier_rmse"]), rel=1e-6)
        assert np.allclose(got.transformation_, ref["T"].reshape(4, 4), rtol=0, atol=TOL_T)
        # the fused synchronous call as well
        poses = synth.hypotheses(12)
        res, sizes = api.refine_batch(model, poses, W, H, scenario["proj"], K, a, api.ICPConvergenceCriteria(0.0, 0.0, 4))
        ores, osizes, _ = O.refine_batch(scenario["tris"], poses, W, H, O.compute_proj(K, W, H), K, ob, (0.0, 0.0, 4), O.SUM_CANONICAL, api.get_option("points_per_block"))
        assert np.array_equal(sizes, osizes) and np.array_equal(res["fitness"], ores["fitness"])
        assert np.allclose(res["T"], ores["T"], rtol=0, atol=TOL_T)
    finally:
        api.set_option("solve", api.SOLVE_HOST)
