"""GPU tests (-m gpu) of pr_compose_detections / pr_compose_detections_multi: labels, front depth, the per-hypothesis records and the frame record
equal the numpy reference over the oracle's renders (tests/compose_ref.py) element for element, the scores are pr_score_poses' bytes and the
sums of the records meet -- int32 and uint16 scenes, ties, duplicates, ROI windows, an odd frame width, two depth chunks, mixed batches, a
batch of two launches over its boxes."""
import threading

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from compose_ref import Composite, assert_composites_equal, check_invariants, compose_ref
from gpu_common import W, H, pathological_hypotheses
from select_ref import PLANTED_SELECTION, planted_frame
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import launch_split_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)                                  # configs[1] sampler


@pytest.fixture(scope="module")
def noisy_scene(scenario):
    """test_select_gpu.py's kind of scene: depth[1] with holes, +-k mm perturbations, a wall behind and clutter in front of the object."""
    rng = np.random.default_rng(20)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    bg = d == 0
    d[bg & (rng.random(d.shape) < 0.5)] = 900
    d[bg & (rng.random(d.shape) < 0.1)] = 150
    d[rng.random(d.shape) < 0.08] = 0
    return d.astype(np.int32)


@pytest.fixture(scope="module")
def renders256(scenario, hyps):
    return O.render(scenario["tris"], hyps, W, H, scenario["proj"])


def _got(out, width=W, height=H):
    labels, depth, scores, visible, frame = out
    return Composite(None if labels is None else labels.to_host().reshape(height, width), None if depth is None else depth.to_host().reshape(height, width),
                     visible, frame, None), scores


def _check(out, want, score_bytes, width=W, height=H):
    got, scores = _got(out, width, height)
    assert_composites_equal(got, want)
    assert scores.tobytes() == score_bytes
    if got.labels is not None and got.depth is not None:
        check_invariants(got, scores)
    return got, scores


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tau", [0, 5, 40])
def test_parity_256_hypotheses(gpu, model, scenario, hyps, noisy_scene, renders256, tau, dtype):
    scene = np.ascontiguousarray(noisy_scene.astype(dtype))
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    pj = scenario["proj"]
    want = compose_ref(renders256, scene, tau)
    tie = want.ties > 1
    assert tie.sum() > 1000 and want.ties.max() >= 3              # the tie rule is what is being tested
    assert np.count_nonzero(want.visible["owned"]) > 50
    check_invariants(want)
    sc = api.score_poses(model, hyps, W, H, pj, sd, tau)
    got, _ = _check(api.compose_detections(model, hyps, W, H, pj, sd, tau), want, sc.tobytes())
    # the reversed batch: its own reference, and the same owner up to the renumbering everywhere but at the ties
    rwant = compose_ref(renders256[::-1], scene, tau)
    rgot, _ = _check(api.compose_detections(model, hyps[::-1], W, H, pj, sd, tau), rwant, sc[::-1].tobytes())
    drawn = got.labels != api.COMPOSE_NONE
    assert np.array_equal(rgot.depth, got.depth)
    assert np.array_equal((rgot.labels.astype(np.int64) != 255 - got.labels.astype(np.int64)) & drawn, tie)
    assert rgot.frame.tobytes() == got.frame.tobytes()


def test_duplicates(gpu, model, scenario, hyps, noisy_scene):
    """Poses [p, p, q, p]: hypothesis 0 owns every pixel of p's render that q does not take, 1 and 3 own nothing."""
    poses = np.stack([hyps[1], hyps[1], hyps[40], hyps[1]])
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    want = compose_ref(r, noisy_scene, 5)
    sc = api.score_poses(model, poses, W, H, scenario["proj"], noisy_scene, 5)
    got, _ = _check(api.compose_detections(model, poses, W, H, scenario["proj"], noisy_scene, 5), want, sc.tobytes())
    p, q = r[0].astype(np.int64), r[2].astype(np.int64)
    q_takes = (q > 0) & ((p <= 0) | (q < p))
    assert np.array_equal(got.labels == 0, (p > 0) & ~q_takes) and np.array_equal(got.labels == 2, q_takes)
    assert got.visible["owned"][1] == 0 and got.visible["owned"][3] == 0 and got.visible["owned"][0] > 0 and got.visible["owned"][2] > 0
    assert ((p > 0) & (q > 0)).sum() > 1000                       # the two renders do overlap


ROIS = [(200, 150, 200, 180), (0, 100, 330, 200), (W - 320, 100, 320, 200), (321, 200, 62, 90), (320, 200, 64, 64)]


@pytest.mark.parametrize("roi", ROIS)
def test_roi_windows(gpu, model, scenario, hyps, noisy_scene, roi):
    poses = hyps[:64]
    pj = scenario["proj"]
    renders = O.render(scenario["tris"], poses, W, H, pj, roi)
    lib = _lib.load()
    td = model.device_tris()
    pp = np.ascontiguousarray(poses, np.float32)
    pjc = np.ascontiguousarray(pj, np.float32)
    for dt in (np.int32, np.uint16):
        scene = np.ascontiguousarray(noisy_scene.astype(dt))
        sd = api.DeviceVector.from_host(scene.reshape(-1))
        want = compose_ref(renders, scene, 10, roi)
        sc = api.score_poses(model, poses, W, H, pj, sd, 10, roi=roi)
        # the caller's buffers start as garbage: every pixel of both is written, outside the window too
        labels = api.DeviceVector.from_host(np.full(W * H, 0x1234, np.uint16))
        depth = api.DeviceVector.from_host(np.full(W * H, -77, np.int32))
        out, vis, frame = np.zeros(64, api.SCORE), np.zeros(64, api.VISIBLE), np.zeros(1, api.FRAME)
        _lib.check(lib.pr_compose_detections(td.data(), td.size() // 9, pp.ctypes.data, 64, W, H, pjc.ctypes.data, _lib.Roi(*roi), sd.data(),
                                             int(dt == np.int32), 10, labels.data(), depth.data(), out.ctypes.data, vis.ctypes.data, frame.ctypes.data))
        got, _ = _check((labels, depth, out, vis, frame[0]), want, sc.tobytes())
        x, y, w, h = roi
        outside = np.ones((H, W), bool)
        outside[y:y + h, x:x + w] = False
        assert (got.labels[outside] == api.COMPOSE_NONE).all() and (got.depth[outside] == 0).all()
        assert got.frame["window"] == w * h and got.frame["covered"] > 0
        _check(api.compose_detections(model, poses, W, H, pj, sd, 10, roi=roi), want, sc.tobytes())


def test_odd_width_narrow_boxes_and_the_last_column(gpu, model, scenario):
    """test_select_gpu.py's 600 x 400 frame and poses: boxes inside one 64-column tile, boxes that straddle a tile boundary, boxes cut by
    each edge of the frame, and the cut last tile (columns 576 .. 599)."""
    Wo, Ho = 600, 400
    K = np.array([572.4114, 0, 300, 0, 573.57043, 200, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Wo, Ho)
    S = synth.scene_pose()

    def at(x, y, z):
        p = S.copy()
        p[:3, 3] = (x, y, z)
        return p

    one_word = [at(x, y, 3000.0) for x in (-63.0, -58.0, -70.0) for y in (0.0, 12.0)]
    straddle = [at(x, 5.0, 3000.0) for x in (100.0, 105.0, 270.0)] + [at(-20.0, 0.0, 2000.0), at(-30.0, 8.0, 2000.0)]
    edges = [at(380.0, 0.0, 800.0), at(385.0, 10.0, 800.0), at(300.0, 100.0, 700.0), at(-380.0, 0.0, 800.0), at(-375.0, -8.0, 800.0),
             at(0.0, -260.0, 800.0), at(10.0, -255.0, 800.0), at(0.0, 262.0, 800.0), at(1560.0, 0.0, 3000.0), at(1555.0, 4.0, 3000.0)]
    near = [at(0.0, 0.0, 250.0), at(5.0, 5.0, 260.0), at(20.0, 20.0, 320.0)]
    poses = np.stack(one_word + straddle + edges + near).astype(np.float32)
    renders = O.render(scenario["tris"], poses, Wo, Ho, proj)
    cols = [np.flatnonzero((r > 0).any(0)) for r in renders]
    assert all(len(c) > 0 for c in cols)
    assert sum(c[-1] == Wo - 1 for c in cols) >= 4 and sum(c[0] == 0 for c in cols) >= 2      # cut by the last and by the first column
    assert any(c[0] >= 576 for c in cols)                         # a box entirely inside the cut last tile
    assert any(c[0] >> 6 == c[-1] >> 6 for c in cols) and any(c[0] >> 6 != c[-1] >> 6 and len(c) < 64 for c in cols)
    r = renders.astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    rng = np.random.default_rng(3)
    scene = scene + np.where(rng.random(scene.shape) < 0.3, rng.integers(-6, 7, scene.shape), 0) * (scene > 0)
    scene[rng.random(scene.shape) < 0.05] = 0
    for dt in (np.int32, np.uint16):
        sce = np.ascontiguousarray(scene.astype(dt))
        for tau in (0, 4, 3000):
            want = compose_ref(renders, sce, tau)
            sc = api.score_poses(model, poses, Wo, Ho, proj, sce, tau)
            got, _ = _check(api.compose_detections(model, poses, Wo, Ho, proj, sce, tau), want, sc.tobytes(), Wo, Ho)
    assert (got.labels[:, Wo - 1] != api.COMPOSE_NONE).any() and (got.labels[:, 0] != api.COMPOSE_NONE).any()
    assert 8 <= np.count_nonzero(got.visible["owned"]) < len(poses)     # the near ones hide some of the far ones, not all


def test_two_depth_chunks(gpu, model, scenario):
    """An 8192 x 2048 frame: 70 hypotheses are two chunks of the depth workspace (64 + 6).  The key frame must carry the first chunk's owners
    into the second launch, and the boxes of the first chunk must survive for the counts."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    poses = synth.hypotheses(70, seed=9)
    scene = O.render(scenario["tris"], synth.scene_pose()[None], Wb, Hb, proj)[0]
    rng = np.random.default_rng(2)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    late = np.zeros((Hb, Wb), bool)                               # pixels that a hypothesis of the second chunk renders

    def one_by_one():
        for i in range(len(poses)):
            r = O.render(scenario["tris"], poses[i:i + 1], Wb, Hb, proj)[0]
            if i >= 64:
                np.logical_or(late, r > 0, out=late)
            yield r

    want = compose_ref(one_by_one(), scene, 4)
    drawn = want.labels != api.COMPOSE_NONE
    assert (want.labels[drawn] >= 64).sum() > 1000                # owned from the second chunk
    assert (late & drawn & (want.labels < 64)).sum() > 1000       # covered by a second-chunk box, kept by a first-chunk owner
    sc = api.score_poses(model, poses, Wb, Hb, proj, sd, 4)
    _check(api.compose_detections(model, poses, Wb, Hb, proj, sd, 4), want, sc.tobytes(), Wb, Hb)


def _rigid(tris, angle, t):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    return np.ascontiguousarray((tris.reshape(-1, 3) @ R.T + np.asarray(t, np.float32)).astype(np.float32).reshape(-1, 3, 3))


@pytest.mark.parametrize("assign", ["interleaved", "random"])
def test_mixed_batch(gpu, scenario, hyps, noisy_scene, assign):
    """Four meshes; mesh 1 is a separate buffer with mesh 0's triangles and the same pose sits at caller index 5 (mesh 1) and 9 (mesh 0):
    grouping by mesh puts 9 first, the owner of their pixels must still be 5."""
    t = scenario["tris"]
    meshes = [t, t.copy(), np.ascontiguousarray(t * np.float32(0.8)), np.ascontiguousarray(t[::3])]
    poses = hyps[:96].copy()
    idx = np.arange(96) % 4 if assign == "interleaved" else np.random.default_rng(7).integers(0, 4, 96)
    idx[5], idx[9] = 1, 0
    poses[5] = poses[9] = _shifted(hyps[200], -40.0)
    for roi in ((0, 0, 0, 0), (200, 150, 200, 180)):
        rr = np.zeros((96, roi[3] or H, roi[2] or W), np.int32)  # every hypothesis rendered by the oracle with its own mesh
        for m in range(4):
            sel = np.flatnonzero(idx == m)
            rr[sel] = O.render(meshes[m], poses[sel], W, H, scenario["proj"], roi)
        assert np.array_equal(rr[5], rr[9])
        want = compose_ref(rr, noisy_scene, 10, roi)
        assert want.visible["owned"][5] > 100 and want.visible["owned"][9] == 0
        assert len(set(idx[np.flatnonzero(want.visible["owned"])])) == 4      # every mesh owns pixels
        sc = api.score_poses_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, 10, roi=roi)
        _check(api.compose_detections_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, 10, roi=roi), want, sc.tobytes())


def _shifted(pose, dz):
    p = pose.copy()
    p[2, 3] += dz
    return p


def test_mixed_batch_of_one_mesh_is_the_single_mesh_call(gpu, model, scenario, hyps, noisy_scene):
    single = _got(api.compose_detections(model, hyps[:70], W, H, scenario["proj"], noisy_scene, 5))
    for meshes, idx in (([model], np.zeros(70, np.int64)), ([scenario["tris"][:10], model, model], np.full(70, 2)),
                        ([model, model], np.arange(70) % 2)):
        multi = _got(api.compose_detections_multi(meshes, idx, hyps[:70], W, H, scenario["proj"], noisy_scene, 5))
        assert_composites_equal(multi[0], single[0])
        assert multi[1].tobytes() == single[1].tobytes()


def test_edge_inputs(gpu, model, scenario, noisy_scene):
    """NaN / infinite / zero matrices, off-frame, behind the camera, a giant, a speck; an empty mesh; batches of one, two and three."""
    pj = scenario["proj"]
    bad, idx_bad = pathological_hypotheses(synth.hypotheses(40, seed=3))
    renders = O.render(scenario["tris"], bad, W, H, pj)
    sc = api.score_poses(model, bad, W, H, pj, noisy_scene, 10)
    got, _ = _check(api.compose_detections(model, bad, W, H, pj, noisy_scene, 10), compose_ref(renders, noisy_scene, 10), sc.tobytes())
    assert sum(got.visible["owned"][i] == 0 for i in idx_bad) >= 8
    none = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    got, scores = _got(api.compose_detections(none, bad[:7], W, H, pj, noisy_scene, 10))
    assert (got.labels == api.COMPOSE_NONE).all() and not got.depth.any() and not got.visible["owned"].any() and not scores["visible"].any()
    assert got.frame["covered"] == 0 and got.frame["window"] == W * H and got.frame["measured"] == (noisy_scene > 0).sum()
    hy = synth.hypotheses(8, seed=5)
    for n in (1, 2, 3):
        r = O.render(scenario["tris"], hy[1:1 + n], W, H, pj)
        sc = api.score_poses(model, hy[1:1 + n], W, H, pj, noisy_scene, 5)
        _check(api.compose_detections(model, hy[1:1 + n], W, H, pj, noisy_scene, 5), compose_ref(r, noisy_scene, 5), sc.tobytes())


def test_workspace_reuse(gpu, model, scenario, hyps, noisy_scene):
    """640 x 480, then 600 x 400, then 640 x 480 again: the key frame of a call owes nothing to the one before."""
    pj = scenario["proj"]

    def big():
        (c, sc) = _got(api.compose_detections(model, hyps[:48], W, H, pj, noisy_scene, 5))
        return c.labels.tobytes(), c.depth.tobytes(), c.visible.tobytes(), c.frame.tobytes(), sc.tobytes()

    first = big()
    Wo, Ho = 600, 400
    K = np.array([572.4114, 0, 300, 0, 573.57043, 200, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Wo, Ho)
    poses = synth.hypotheses(20, seed=2)
    small_scene = np.ascontiguousarray(noisy_scene[:Ho, :Wo])
    want = compose_ref(O.render(scenario["tris"], poses, Wo, Ho, proj), small_scene, 5)
    sc = api.score_poses(model, poses, Wo, Ho, proj, small_scene, 5)
    _check(api.compose_detections(model, poses, Wo, Ho, proj, small_scene, 5), want, sc.tobytes(), Wo, Ho)
    assert big() == first
    assert first[0] == compose_ref(O.render(scenario["tris"], hyps[:48], W, H, pj), noisy_scene, 5).labels.tobytes()


def test_arguments_and_limits(gpu, model, scenario, hyps, noisy_scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    roi0 = _lib.Roi(0, 0, 0, 0)
    poses = hyps[:12]
    want = compose_ref(O.render(scenario["tris"], poses, W, H, pj), noisy_scene, 5)
    sc = api.score_poses(model, poses, W, H, pj, noisy_scene, 5)
    # either device output may be left out
    for wl, wd in ((True, False), (False, True), (False, False)):
        out = api.compose_detections(model, poses, W, H, pj, noisy_scene, 5, want_labels=wl, want_depth=wd)
        assert (out[0] is not None) == wl and (out[1] is not None) == wd
        _check(out, want, sc.tobytes())
    # no hypotheses: PR_OK, nothing written (null pointers allowed)
    assert lib.pr_compose_detections(None, 0, None, 0, W, H, pj.ctypes.data, roi0, None, 1, 5, None, None, None, None, None) == _lib.PR_OK
    assert lib.pr_compose_detections_multi(None, 0, None, None, 0, W, H, pj.ctypes.data, roi0, None, 1, 5, None, None, None, None, None) == _lib.PR_OK
    out = api.compose_detections(model, np.zeros((0, 4, 4), np.float32), W, H, pj, noisy_scene, 5)
    assert out[0] is None and out[1] is None and len(out[2]) == 0 and len(out[3]) == 0 and not any(out[4][f] for f in ("window", "measured", "covered"))
    out = api.compose_detections_multi([model], np.zeros(0, np.int64), np.zeros((0, 4, 4), np.float32), W, H, pj, noisy_scene, 5)
    assert out[0] is None and len(out[2]) == 0
    # one more than PR_COMPOSE_MAX_POSES is refused before anything runs, the limit in the message
    many = np.ascontiguousarray(np.broadcast_to(hyps[1], (65536, 4, 4)), np.float32)
    with pytest.raises(api.PoseRefineError) as e:
        api.compose_detections(model, many, W, H, pj, noisy_scene, 5, want_labels=False, want_depth=False)
    assert e.value.code == _lib.PR_ERR_INVALID and "65535" in str(e.value) and "PR_COMPOSE_MAX_POSES" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:
        api.compose_detections_multi([model], np.zeros(65536, np.int64), many, W, H, pj, noisy_scene, 5, want_labels=False, want_depth=False)
    assert e.value.code == _lib.PR_ERR_INVALID and "PR_COMPOSE_MAX_POSES" in str(e.value)
    # pr_score_poses' checks: tau < 0, a ROI outside the image
    with pytest.raises(api.PoseRefineError) as e:
        api.compose_detections(model, poses, W, H, pj, noisy_scene, -1)
    assert e.value.code == _lib.PR_ERR_INVALID
    with pytest.raises(api.PoseRefineError) as e:
        api.compose_detections(model, poses, W, H, pj, noisy_scene, 5, roi=(600, 0, 100, 100))
    assert e.value.code == _lib.PR_ERR_INVALID and "roi out of image" in str(e.value)
    # a null scene and null record pointers: refused with nothing written, on the host or on the device
    td = model.device_tris()
    pp = np.ascontiguousarray(poses, np.float32)
    sd = api.DeviceVector.from_host(noisy_scene.reshape(-1))
    labels = api.DeviceVector.from_host(np.full(W * H, 0x1234, np.uint16))
    depth = api.DeviceVector.from_host(np.full(W * H, -77, np.int32))
    out, vis, frame = np.zeros(12, api.SCORE), np.zeros(12, api.VISIBLE), np.zeros(1, api.FRAME)
    table = (_lib.MeshRef * 1)(_lib.MeshRef(td.data(), td.size() // 9))
    idx = np.zeros(12, np.uint32)
    for scene_p, sc_p, vis_p, fr_p in ((None, out.ctypes.data, vis.ctypes.data, frame.ctypes.data), (sd.data(), None, vis.ctypes.data, frame.ctypes.data),
                                       (sd.data(), out.ctypes.data, None, frame.ctypes.data), (sd.data(), out.ctypes.data, vis.ctypes.data, None)):
        assert lib.pr_compose_detections(td.data(), td.size() // 9, pp.ctypes.data, 12, W, H, pj.ctypes.data, roi0, scene_p, 1, 5, labels.data(), depth.data(),
                                         sc_p, vis_p, fr_p) == _lib.PR_ERR_INVALID
        assert lib.pr_compose_detections_multi(table, 1, idx.ctypes.data, pp.ctypes.data, 12, W, H, pj.ctypes.data, roi0, scene_p, 1, 5, labels.data(),
                                               depth.data(), sc_p, vis_p, fr_p) == _lib.PR_ERR_INVALID
    assert not out["visible"].any() and not vis["owned"].any() and not frame["window"].any()
    assert (labels.to_host() == 0x1234).all() and (depth.to_host() == -77).all()


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_compose_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, noisy_scene, solve):
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
        alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        alone = _got(api.compose_detections(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5))
        api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        mid = _got(api.compose_detections(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5))
        res, sizes = api.refine_wait(0)
        assert_composites_equal(mid[0], alone[0])
        assert mid[1].tobytes() == alone[1].tobytes() and mid[0].visible.tobytes() == alone[0].visible.tobytes()
        assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()
    finally:
        api.set_option("solve", before)


def test_private_context_gives_the_same_bytes(gpu, model, scenario, hyps, noisy_scene):
    shared = _got(api.compose_detections(model, hyps, W, H, scenario["proj"], noisy_scene, 5))
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                box["out"] = _got(api.compose_detections(model, hyps, W, H, scenario["proj"], noisy_scene, 5))
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert_composites_equal(box["out"][0], shared[0])
    assert box["out"][1].tobytes() == shared[1].tobytes() and box["out"][0].frame.tobytes() == shared[0].frame.tobytes()


def test_planted_frame_end_to_end(gpu, model, scenario):
    """score_overlap -> select_hypotheses -> compose the detections: every one owns pixels and the labels are the reference's."""
    scene, poses = planted_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    sc, ov = api.score_overlap(model, poses, W, H, scenario["proj"], sd, 5)
    sel = api.select_hypotheses(sc, ov)
    assert sel.tolist() == PLANTED_SELECTION
    want = compose_ref(O.render(scenario["tris"], poses[sel], W, H, scenario["proj"]), scene, 5)
    got, scores = _check(api.compose_detections(model, poses[sel], W, H, scenario["proj"], sd, 5), want, sc[sel].tobytes())
    assert (got.visible["owned"] > 0).all() and sorted(np.unique(got.labels).tolist()) == [0, 1, 2, api.COMPOSE_NONE]
    frac = api.visible_fraction(scores, got.visible)
    assert frac[0] == 1.0 and frac[1] > 0.99 and 0.7 < frac[2] < 0.8      # instance 0 (last here) stands behind instance 1
    assert int(got.frame["explained"]) / int(got.frame["covered"]) == int(want.frame["explained"]) / int(want.frame["covered"]) > 0.8


def test_batch_of_two_box_launches(gpu):
    """verify_ref.launch_split_case at 32768 + 5 hypotheses (below PR_COMPOSE_MAX_POSES): the launches over the boxes are split in two, and
    the second's keys carry indices above 32767.  Ties go to the lower index, so every label is below 8 and every later duplicate owns
    nothing; the records behind the split are the reference's.  Behind the split every hypothesis takes the next pose
    (seam_cases.seam_index), and the reference is composed from the stack so indexed: hypothesis 32768 + j never expects hypothesis j's."""
    c = launch_split_case()
    P = c["P"]
    assert P <= api.COMPOSE_MAX_POSES
    idx = seam_index(P, 8)
    poses = c["poses"][idx]
    want = compose_ref((c["renders"][idx[i]] for i in range(P)), c["scene"], c["tau"])
    out = api.compose_detections(c["tris"], poses, c["W"], c["H"], c["proj"], c["scene"], c["tau"])
    got, scores = _got(out, c["W"], c["H"])
    assert_composites_equal(got, want)
    check_invariants(got, scores)
    assert_seam_visible(c["scores"], idx)
    assert_records_take(scores, c["scores"], idx)
    drawn = got.labels != api.COMPOSE_NONE
    assert drawn.any() and (got.labels[drawn] < 8).all()
    assert not got.visible["owned"][8:].any() and got.visible["owned"][:8].sum() == got.frame["covered"] > 0
    assert got.visible[32768:].tobytes() == want.visible[32768:].tobytes() == bytes(want.visible[32768:].nbytes)
    assert (want.ties[drawn] >= P // 8).all()
