"""GPU tests (-m gpu) of pr_score_overlap / pr_score_overlap_multi: the scores are pr_score_poses' bytes and the P x P matrix of shared
inlier pixels equals the numpy reference over the oracle's renders (tests/select_ref.py) element for element -- int32 and uint16 scenes,
ROI windows, odd frame widths, boxes inside one 64-pixel word and at the frame's edge, batches of several depth chunks, mixed batches --
and the planted frame comes back as exactly its three instances."""
import threading

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H, pathological_hypotheses
from select_ref import PLANTED_SELECTION, overlap_ref, planted_frame
from verify_ref import assert_scores_equal, score_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)                                  # configs[1] sampler


@pytest.fixture(scope="module")
def noisy_scene(scenario):
    """test_verify_gpu.py's kind of scene: depth[1] with holes, +-k mm perturbations, a wall behind and clutter in front of the object."""
    rng = np.random.default_rng(20)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    bg = d == 0
    d[bg & (rng.random(d.shape) < 0.5)] = 900
    d[bg & (rng.random(d.shape) < 0.1)] = 150
    d[rng.random(d.shape) < 0.08] = 0
    return d.astype(np.int32)


def _assert_overlap(got_sc, got_ov, want_sc, want_ov):
    assert_scores_equal(got_sc, want_sc)
    assert got_ov.dtype == np.uint32 and got_ov.shape == want_ov.shape
    bad = np.argwhere(got_ov != want_ov)
    assert len(bad) == 0, (len(bad), bad[:10], got_ov[tuple(bad[:10].T)], want_ov[tuple(bad[:10].T)])
    assert np.array_equal(got_ov, got_ov.T)
    assert np.array_equal(np.diag(got_ov), got_sc["inlier"])


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tau", [0, 5, 40])
def test_parity_256_hypotheses(gpu, model, scenario, hyps, noisy_scene, tau, dtype):
    scene = np.ascontiguousarray(noisy_scene.astype(dtype))
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    sc, ov = api.score_overlap(model, hyps, W, H, scenario["proj"], sd, tau)
    assert sc.tobytes() == api.score_poses(model, hyps, W, H, scenario["proj"], sd, tau).tobytes()
    renders = O.render(scenario["tris"], hyps, W, H, scenario["proj"])
    _assert_overlap(sc, ov, score_ref(renders, scene, tau), overlap_ref(renders, scene, tau))
    assert np.count_nonzero(np.triu(ov, 1)) > 10000               # the pairs do share pixels
    # a second call into the same workspaces gives the same bytes (words of the planes that a box does not cover are never read)
    sc2, ov2 = api.score_overlap(model, hyps[::-1], W, H, scenario["proj"], sd, tau)
    assert sc2.tobytes() == sc[::-1].tobytes() and np.array_equal(ov2, ov[::-1, ::-1])


@pytest.mark.parametrize("P", [513, 1101])
def test_larger_batches(gpu, model, scenario, noisy_scene, P):
    """Odd batch sizes above 256: two workgroups per hypothesis (513) and one (1101) in the pair kernel, every pair with exactly one owner."""
    poses = synth.hypotheses(P, seed=12)
    sc, ov = api.score_overlap(model, poses, W, H, scenario["proj"], noisy_scene, 5)
    assert sc.tobytes() == api.score_poses(model, poses, W, H, scenario["proj"], noisy_scene, 5).tobytes()
    parts = [O.render(scenario["tris"], poses[i:i + 128], W, H, scenario["proj"]) for i in range(0, P, 128)]
    want_sc = np.concatenate([score_ref(r, noisy_scene, 5) for r in parts])
    want_ov = overlap_ref((r for part in parts for r in part), noisy_scene, 5)
    _assert_overlap(sc, ov, want_sc, want_ov)
    assert np.count_nonzero(np.triu(ov, 1)) > P * P // 4


ROIS = [(200, 150, 200, 180), (0, 0, W, H), (0, 100, 330, 200), (100, 0, 300, 240), (W - 320, 100, 320, 200), (100, H - 240, 300, 240),
        (300, 230, 60, 40), (321, 200, 62, 90), (320, 200, 64, 64)]


@pytest.mark.parametrize("roi", ROIS)
def test_roi_parity(gpu, model, scenario, hyps, noisy_scene, roi):
    poses = hyps[:64]
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"], roi)
    for dt in (np.int32, np.uint16):
        scene = np.ascontiguousarray(noisy_scene.astype(dt))
        sc, ov = api.score_overlap(model, poses, W, H, scenario["proj"], scene, 10, roi=roi)
        assert sc.tobytes() == api.score_poses(model, poses, W, H, scenario["proj"], scene, 10, roi=roi).tobytes()
        _assert_overlap(sc, ov, score_ref(renders, scene, 10, roi), overlap_ref(renders, scene, 10, roi))
    assert ov.max() > 0


def test_pathological_hypotheses(gpu, model, scenario, noisy_scene):
    """NaN / infinite / zero matrices, off-frame, behind the camera, a giant, a speck: zero rows and columns, everything else as without them."""
    bad, idx_bad = pathological_hypotheses(synth.hypotheses(40, seed=3))
    sc, ov = api.score_overlap(model, bad, W, H, scenario["proj"], noisy_scene, 10)
    assert sc.tobytes() == api.score_poses(model, bad, W, H, scenario["proj"], noisy_scene, 10).tobytes()
    renders = O.render(scenario["tris"], bad, W, H, scenario["proj"])
    _assert_overlap(sc, ov, score_ref(renders, noisy_scene, 10), overlap_ref(renders, noisy_scene, 10))
    empty = [i for i in idx_bad if sc["inlier"][i] == 0]
    assert len(empty) >= 8
    assert not ov[empty].any() and not ov[:, empty].any()
    # an empty mesh: a matrix of zeros
    none = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    sc, ov = api.score_overlap(none, bad[:7], W, H, scenario["proj"], noisy_scene, 10)
    assert not ov.any() and not sc["visible"].any()


def _box_columns(tris, pose, K):
    """Columns the hypothesis' pixel box may reach: the mesh box's corners through the pose and the intrinsics, padded by 3 pixels."""
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    c = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    p = c @ pose.astype(np.float64).T
    u = K[0] * p[:, 0] / p[:, 2] + K[2]
    return int(np.floor(u.min())) - 3, int(np.ceil(u.max())) + 3


def test_odd_width_narrow_boxes_and_the_last_column(gpu, model, scenario):
    """A 600 x 400 frame (the last 64-pixel word of a row is cut at pixel 599): far hypotheses whose boxes begin and end inside one word, ones
    that straddle a word boundary, ones cut by each edge of the frame (the last column included), and near ones that cover them all."""
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
    tris = scenario["tris"]
    for p in one_word:
        c0, c1 = _box_columns(tris, p, K)
        assert c0 >> 6 == c1 >> 6 == 4, (c0, c1)                  # inside word 4 (columns 256 .. 319), padding included
    renders = O.render(tris, poses, Wo, Ho, proj)
    cols = [np.flatnonzero((r > 0).any(0)) for r in renders]
    assert all(len(c) > 0 for c in cols)
    assert sum(c[-1] == Wo - 1 for c in cols) >= 4 and sum(c[0] == 0 for c in cols) >= 2      # cut by the last and by the first column
    assert any(c[0] >= 576 for c in cols)                         # a box entirely inside the cut last word
    r = renders.astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    rng = np.random.default_rng(3)
    scene = scene + np.where(rng.random(scene.shape) < 0.3, rng.integers(-6, 7, scene.shape), 0) * (scene > 0)
    scene[rng.random(scene.shape) < 0.05] = 0
    for dt in (np.int32, np.uint16):
        sce = np.ascontiguousarray(scene.astype(dt))
        for tau in (0, 4, 3000):
            sc, ov = api.score_overlap(model, poses, Wo, Ho, proj, sce, tau)
            assert sc.tobytes() == api.score_poses(model, poses, Wo, Ho, proj, sce, tau).tobytes()
            _assert_overlap(sc, ov, score_ref(renders, sce, tau), overlap_ref(renders, sce, tau))
    assert (np.diag(ov) > 0).all()                                # tau = 3000: every hypothesis keeps pixels, the far ones under the near ones too
    assert ov[0, len(poses) - 3] > 0


def test_batch_of_several_depth_chunks(gpu, model, scenario):
    """test_chunked_batch_matches_small_batches' 8192 x 2048 frame: 150 hypotheses span three chunks of the depth workspace; the planes and
    boxes of a chunk must survive the next one, and pairs across chunks must be right (a box here needs row bands in the pair kernel)."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    poses = synth.hypotheses(150, seed=9)
    scene = O.render(scenario["tris"], synth.scene_pose()[None], Wb, Hb, proj)[0]
    rng = np.random.default_rng(2)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    sc, ov = api.score_overlap(model, poses, Wb, Hb, proj, sd, 4)
    assert sc.tobytes() == api.score_poses(model, poses, Wb, Hb, proj, sd, 4).tobytes()
    one_by_one = (O.render(scenario["tris"], poses[i:i + 1], Wb, Hb, proj)[0] for i in range(len(poses)))
    want = overlap_ref(one_by_one, scene, 4)
    assert np.array_equal(ov, want)
    assert np.array_equal(np.diag(ov), sc["inlier"]) and np.array_equal(ov, ov.T)
    assert np.count_nonzero(ov[:64, 128:]) > 64 * 22 // 2         # first chunk against the last one: pairs that share pixels


def test_boxes_larger_than_one_lds_band(gpu, model, scenario):
    """Close-ups in a 2048 x 1536 frame: a box of more than 6144 words (48 KB) goes through the pair kernel in bands of rows, and what a
    band adds to a matrix element must land on what the bands before it left there."""
    Wc, Hc = 2048, 1536
    K = np.array([1200.0, 0, Wc / 2, 0, 1200.0, Hc / 2, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Wc, Hc)
    S = synth.scene_pose()
    base = synth.hypotheses(14, seed=4)[1:]
    poses = base.copy()
    poses[:, :3, 3] += np.array([[-20 + 3 * i, -20 + 2 * i, -200.0 + 5 * i] for i in range(13)], np.float32)         # z from 120 to 180 mm
    poses = np.concatenate([poses, base[:3]])                     # and three at the usual distance, inside the close-ups' boxes
    renders = O.render(scenario["tris"], poses, Wc, Hc, proj)
    words = [(np.ptp(np.flatnonzero((r > 0).any(0)) >> 6) + 1) * (np.ptp(np.flatnonzero((r > 0).any(1))) + 1) for r in renders]
    assert sum(w > 2 * 6144 for w in words) >= 5 and sum(w > 6144 for w in words) >= 10 and min(words) < 6144
    near = S.copy()
    near[2, 3] = 150.0
    scene = O.render(scenario["tris"], near[None], Wc, Hc, proj)[0].astype(np.int64)
    rng = np.random.default_rng(6)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    for tau in (6, 40, 200):
        sc, ov = api.score_overlap(model, poses, Wc, Hc, proj, scene, tau)
        _assert_overlap(sc, ov, score_ref(renders, scene, tau), overlap_ref(renders, scene, tau))
    assert np.count_nonzero(np.triu(ov, 1)) > 100


def _rigid(tris, angle, t):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    return np.ascontiguousarray((tris.reshape(-1, 3) @ R.T + np.asarray(t, np.float32)).astype(np.float32).reshape(-1, 3, 3))


@pytest.mark.parametrize("assign", ["interleaved", "random"])
def test_mixed_batch(gpu, scenario, hyps, noisy_scene, assign):
    t = scenario["tris"]
    meshes = [t, _rigid(t, 0.3, (4.0, -3.0, 2.0)), np.ascontiguousarray(t * np.float32(0.8)), np.ascontiguousarray(t[::3])]
    poses = hyps[:96]
    idx = np.arange(96) % 4 if assign == "interleaved" else np.random.default_rng(7).integers(0, 4, 96)
    for roi in ((0, 0, 0, 0), (200, 150, 200, 180)):
        rr = np.zeros((96, roi[3] or H, roi[2] or W), np.int32)  # every hypothesis rendered by the oracle with its own mesh
        for m in range(4):
            sel = np.flatnonzero(idx == m)
            rr[sel] = O.render(meshes[m], poses[sel], W, H, scenario["proj"], roi)
        sc, ov = api.score_overlap_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, 10, roi=roi)
        assert sc.tobytes() == api.score_poses_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, 10, roi=roi).tobytes()
        _assert_overlap(sc, ov, score_ref(rr, noisy_scene, 10, roi), overlap_ref(rr, noisy_scene, 10, roi))
    a, b = np.flatnonzero(idx == 0), np.flatnonzero(idx == 3)
    assert ov[np.ix_(a, b)].max() > 0                             # pairs of different meshes do share pixels


def test_mixed_batch_of_one_mesh_is_the_single_mesh_call(gpu, model, scenario, hyps, noisy_scene):
    sc, ov = api.score_overlap(model, hyps[:70], W, H, scenario["proj"], noisy_scene, 5)
    for meshes, idx in (([model], np.zeros(70, np.int64)), ([scenario["tris"][:10], model, model], np.full(70, 2)),
                        ([model, model], np.arange(70) % 2)):
        msc, mov = api.score_overlap_multi(meshes, idx, hyps[:70], W, H, scenario["proj"], noisy_scene, 5)
        assert msc.tobytes() == sc.tobytes() and np.array_equal(mov, ov)


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_overlap_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, noisy_scene, solve):
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
        alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        alone_sc, alone_ov = api.score_overlap(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5)
        api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        mid_sc, mid_ov = api.score_overlap(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5)
        res, sizes = api.refine_wait(0)
        assert mid_sc.tobytes() == alone_sc.tobytes() and np.array_equal(mid_ov, alone_ov)
        assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()
    finally:
        api.set_option("solve", before)


def test_private_context_gives_the_same_matrix(gpu, model, scenario, hyps, noisy_scene):
    shared = api.score_overlap(model, hyps, W, H, scenario["proj"], noisy_scene, 5)
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                box["out"] = api.score_overlap(model, hyps, W, H, scenario["proj"], noisy_scene, 5)
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert box["out"][0].tobytes() == shared[0].tobytes() and np.array_equal(box["out"][1], shared[1])


def test_limits_and_arguments(gpu, model, scenario, hyps, noisy_scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    roi0 = _lib.Roi(0, 0, 0, 0)
    # no hypotheses: PR_OK, nothing written (null pointers allowed)
    assert lib.pr_score_overlap(None, 0, None, 0, W, H, pj.ctypes.data, roi0, None, 1, 5, None, None) == _lib.PR_OK
    sc, ov = api.score_overlap(model, np.zeros((0, 4, 4), np.float32), W, H, pj, noisy_scene, 5)
    assert len(sc) == 0 and ov.shape == (0, 0)
    msc, mov = api.score_overlap_multi([model], np.zeros(0, np.int64), np.zeros((0, 4, 4), np.float32), W, H, pj, noisy_scene, 5)
    assert len(msc) == 0 and mov.shape == (0, 0)
    # one more than PR_OVERLAP_MAX_POSES is refused before anything runs, the limit in the message
    assert api.OVERLAP_MAX_POSES == 4096
    many = np.ascontiguousarray(np.broadcast_to(hyps[1], (4097, 4, 4)), np.float32)
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap(model, many, W, H, pj, noisy_scene, 5)
    assert e.value.code == _lib.PR_ERR_INVALID and "4096" in str(e.value) and "PR_OVERLAP_MAX_POSES" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap_multi([model], np.zeros(4097, np.int64), many, W, H, pj, noisy_scene, 5)
    assert e.value.code == _lib.PR_ERR_INVALID and "4096" in str(e.value)
    # pr_score_poses' checks: tau < 0, a ROI outside the image, a null scene, a null matrix
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap(model, hyps[:4], W, H, pj, noisy_scene, -1)
    assert e.value.code == _lib.PR_ERR_INVALID
    with pytest.raises(api.PoseRefineError) as e:
        api.score_overlap(model, hyps[:4], W, H, pj, noisy_scene, 5, roi=(600, 0, 100, 100))
    assert e.value.code == _lib.PR_ERR_INVALID and "roi out of image" in str(e.value)
    td = model.device_tris()
    pp = np.ascontiguousarray(hyps[:4], np.float32)
    sd = api.DeviceVector.from_host(noisy_scene.reshape(-1))
    out = np.zeros(4, api.SCORE)
    mat = np.full((4, 4), 0xffffffff, np.uint32)
    assert lib.pr_score_overlap(td.data(), td.size() // 9, pp.ctypes.data, 4, W, H, pj.ctypes.data, roi0, None, 1, 5, out.ctypes.data,
                                mat.ctypes.data) == _lib.PR_ERR_INVALID
    assert lib.pr_score_overlap(td.data(), td.size() // 9, pp.ctypes.data, 4, W, H, pj.ctypes.data, roi0, sd.data(), 1, 5, out.ctypes.data,
                                None) == _lib.PR_ERR_INVALID
    assert (mat == 0xffffffff).all() and not out["visible"].any()
    # a batch of one, of two, of three: the smallest pair schedules
    for n in (1, 2, 3):
        sc, ov = api.score_overlap(model, hyps[1:1 + n], W, H, pj, noisy_scene, 5)
        r = O.render(scenario["tris"], hyps[1:1 + n], W, H, pj)
        _assert_overlap(sc, ov, score_ref(r, noisy_scene, 5), overlap_ref(r, noisy_scene, 5))


def test_planted_frame_through_the_device(gpu, model, scenario):
    scene, poses = planted_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    for tau in (5, 10):
        sc, ov = api.score_overlap(model, poses, W, H, scenario["proj"], sd, tau)
        _assert_overlap(sc, ov, score_ref(renders, scene, tau), overlap_ref(renders, scene, tau))
        for ms in ((1, 10), (1, 4), (1, 2)):
            for mf in (0.0, 0.5):
                assert api.select_hypotheses(sc, ov, max_shared=ms, min_fraction=mf).tolist() == PLANTED_SELECTION, (tau, ms, mf)
