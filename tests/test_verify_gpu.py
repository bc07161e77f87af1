"""GPU tests (-m gpu) of pr_score_poses: every hypothesis rendered and compared with the scene depth pixel by pixel, held to a numpy
classifier over the oracle's renders (tests/verify_ref.py) -- every integer field bit-exact, int32 and uint16 scenes, with and without ROI."""
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H, raw_h2d
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import assert_scores_equal, launch_split_case, score_ref

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)                                  # configs[1] sampler


@pytest.fixture(scope="module")
def noisy_scene(scenario):
    """depth[1] with holes (0), +-k mm perturbations and background put in front of / behind where a hypothesis may render."""
    rng = np.random.default_rng(20)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    bg = d == 0
    d[bg & (rng.random(d.shape) < 0.5)] = 900                     # wall far behind the object
    d[bg & (rng.random(d.shape) < 0.1)] = 150                     # clutter in front of it
    d[rng.random(d.shape) < 0.08] = 0                             # holes
    return d.astype(np.int32)


def _scene(scene, dtype):
    return np.ascontiguousarray(scene.astype(dtype))


def test_self_consistency(gpu, model, scenario):
    d1 = scenario["depth"][1]
    for dt in (np.int32, np.uint16):
        sc = api.score_poses(model, scenario["poses"][1][None], W, H, scenario["proj"], _scene(d1, dt), 0)
        n = np.count_nonzero(d1)
        assert n > 0
        assert sc["visible"][0] == n and sc["inlier"][0] == n, (dt, sc)
        for f in ("occluded", "violation", "missing", "reserved", "abs_err_sum"):
            assert sc[f][0] == 0, (dt, f, sc)


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tau", [0, 5, 20])
def test_parity_256_hypotheses(gpu, model, scenario, hyps, noisy_scene, tau, dtype):
    scene = _scene(noisy_scene, dtype)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    got = api.score_poses(model, hyps, W, H, scenario["proj"], sd, tau)
    want = score_ref(O.render(scenario["tris"], hyps, W, H, scenario["proj"]), scene, tau)
    assert_scores_equal(got, want)
    for f in ("inlier", "occluded", "violation", "missing"):      # every class occurs, or the test proves little
        assert got[f].sum() > 0, f
    if tau > 0:
        assert (got["abs_err_sum"] > 0).any()


ROIS_INSIDE = [(200, 150, 200, 180), (0, 0, W, H), (0, 100, 330, 200), (100, 0, 300, 240), (W - 320, 100, 320, 200),
               (100, H - 240, 300, 240), (300, 230, 60, 40)]


@pytest.mark.parametrize("roi", ROIS_INSIDE)
def test_roi_parity(gpu, model, scenario, hyps, noisy_scene, roi):
    poses = hyps[:64]
    for dt in (np.int32, np.uint16):
        scene = _scene(noisy_scene, dt)
        got = api.score_poses(model, poses, W, H, scenario["proj"], scene, 10, roi=roi)
        want = score_ref(O.render(scenario["tris"], poses, W, H, scenario["proj"], roi), scene, 10, roi)
        assert_scores_equal(got, want)
    full = api.score_poses(model, poses, W, H, scenario["proj"], noisy_scene, 10)
    assert (got["visible"] <= full["visible"]).all()
    if roi == (300, 230, 60, 40):                                 # a window that cuts the object
        assert (got["visible"] > 0).any() and (got["visible"] < full["visible"]).all()


@pytest.mark.parametrize("roi", [(600, 0, 100, 100), (-1, 0, 10, 10), (0, 400, 10, 100), (0, -5, 10, 10)])
def test_roi_out_of_image(gpu, model, scenario, hyps, roi):
    with pytest.raises(api.PoseRefineError) as e:
        api.score_poses(model, hyps[:4], W, H, scenario["proj"], scenario["depth"][1], 5, roi=roi)
    assert e.value.code == _lib.PR_ERR_INVALID and "roi out of image" in str(e.value)


def test_visible_equals_refine_cloud_sizes(gpu, model, scenario, hyps, gscenes):
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 1)
    _, sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    sc = api.score_poses(model, hyps, W, H, scenario["proj"], scenario["depth"][1], 5)
    assert np.array_equal(sc["visible"], sizes)
    roi = (220, 160, 150, 120)
    _, rsizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit, roi=roi)
    rsc = api.score_poses(model, hyps, W, H, scenario["proj"], scenario["depth"][1], 5, roi=roi)
    assert np.array_equal(rsc["visible"], rsizes)
    assert (rsizes < sizes).any()


def _median_fraction(sc):
    den = sc["visible"].astype(np.int64) - sc["occluded"]
    return float(np.median(sc["inlier"][den > 0] / den[den > 0]))


def test_refined_poses_end_to_end(gpu, model, scenario, hyps, gscenes, golden_dir):
    d1 = scenario["depth"][1]
    g = np.load(os.path.join(golden_dir, "config1.npz"))
    rec = np.zeros(256, api.RESULT)
    rec["T"] = g["fixed20_T"]
    ref_poses = api.refined_poses(rec, hyps)
    got = api.score_poses(model, ref_poses, W, H, scenario["proj"], d1, 5)
    assert_scores_equal(got, score_ref(O.render(scenario["tris"], ref_poses, W, H, scenario["proj"]), d1, 5))
    # live: refine_batch -> refined_poses -> score_poses
    res, _ = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 20))
    live = api.refined_poses(res, hyps)
    lsc = api.score_poses(model, live, W, H, scenario["proj"], d1, 5)
    assert_scores_equal(lsc, score_ref(O.render(scenario["tris"], live, W, H, scenario["proj"]), d1, 5))
    init = api.score_poses(model, hyps, W, H, scenario["proj"], d1, 5)
    best = api.rank_hypotheses(lsc)[0]
    print(f"median inlier fraction (tau 5 mm): initial {_median_fraction(init):.4f}, refined {_median_fraction(lsc):.4f}; "
          f"best refined hypothesis {best}: {lsc[best]}")


def test_edge_cases(gpu, model, scenario, hyps):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    d1 = scenario["depth"][1]
    # no hypotheses: PR_OK, nothing written (null pointers allowed)
    assert lib.pr_score_poses(None, 0, None, 0, W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0), None, 1, 5, None) == _lib.PR_OK
    assert len(api.score_poses(model, np.zeros((0, 4, 4), np.float32), W, H, pj, d1, 5)) == 0
    # behind the camera / off-screen: all zeros
    odd = np.stack([hyps[1].copy(), hyps[2].copy(), hyps[3].copy()])
    odd[0, 2, 3] = -300.0
    odd[1, 0, 3] = 1.0e6
    sc = api.score_poses(model, odd, W, H, pj, d1, 5)
    for f in ("visible", "inlier", "occluded", "violation", "missing", "abs_err_sum"):
        assert sc[f][0] == 0 and sc[f][1] == 0, f
    assert sc["visible"][2] > 0
    # an empty mesh renders nothing
    empty = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    sc = api.score_poses(empty, hyps[:5], W, H, pj, d1, 5)
    assert all((sc[f] == 0).all() for f in ("visible", "inlier", "occluded", "violation", "missing", "abs_err_sum"))
    # extreme int32 scene values: <= 0 (missing) and near INT32_MAX (no overflow of |r - s|, exact 64-bit sums)
    poses = hyps[:16]
    renders = O.render(scenario["tris"], poses, W, H, pj)
    rng = np.random.default_rng(5)
    ext = rng.choice(np.array([INT32_MAX, INT32_MAX - 1, INT32_MAX - 1000, -1, -INT32_MAX - 1, 0, 300], np.int64), size=(H, W)).astype(np.int32)
    for tau in (0, 1000, INT32_MAX - 1, INT32_MAX):
        got = api.score_poses(model, poses, W, H, pj, ext, tau)
        want = score_ref(renders, ext, tau)
        assert_scores_equal(got, want)
    assert got["abs_err_sum"].max() > 2**40                       # tau = INT32_MAX: the far values are inliers; their sum needs 64 bits
    assert got["missing"].min() > 0
    # tau < 0, null scene
    with pytest.raises(api.PoseRefineError) as e:
        api.score_poses(model, poses, W, H, pj, d1, -1)
    assert e.value.code == _lib.PR_ERR_INVALID
    out = np.zeros(len(poses), api.SCORE)
    td = model.device_tris()
    pp = np.ascontiguousarray(poses, np.float32)
    assert lib.pr_score_poses(td.data(), td.size() // 9, pp.ctypes.data, len(poses), W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0),
                              None, 1, 5, out.ctypes.data) == _lib.PR_ERR_INVALID
    assert lib.pr_score_poses(td.data(), td.size() // 9, pp.ctypes.data, len(poses), W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0),
                              None, 0, 5, out.ctypes.data) == _lib.PR_ERR_INVALID
    assert (out["visible"] == 0).all()


def test_scene_is_read_on_every_call(gpu, model, scenario, hyps, noisy_scene):
    poses = hyps[:64]
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    for dt in (np.int32, np.uint16):
        s1 = _scene(noisy_scene, dt)
        s2 = _scene(scenario["depth"][1], dt)
        s3 = _scene(np.where(noisy_scene > 0, noisy_scene + 7, 0), dt)
        sd = api.DeviceVector.from_host(s1.reshape(-1))
        assert_scores_equal(api.score_poses(model, poses, W, H, scenario["proj"], sd, 5), score_ref(renders, s1, 5))
        _lib.check(_lib.load().pr_memcpy_h2d(sd.data(), s2.ctypes.data, s2.nbytes))           # through the library
        assert_scores_equal(api.score_poses(model, poses, W, H, scenario["proj"], sd, 5), score_ref(renders, s2, 5))
        raw_h2d(sd.data(), s3)                                                               # behind its back
        assert_scores_equal(api.score_poses(model, poses, W, H, scenario["proj"], sd, 5), score_ref(renders, s3, 5))


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_score_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, noisy_scene, solve):
    """A synchronous score while a batch is pending on a slot of the same context (device solve: the slot's own streams; host solve:
    the slot's helper thread): both give what they give alone."""
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        _submit_score_wait(model, scenario, hyps, gscenes, noisy_scene)
    finally:
        api.set_option("solve", before)


def _submit_score_wait(model, scenario, hyps, gscenes, noisy_scene):
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    alone_sc = api.score_poses(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5)
    api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
    mid_sc = api.score_poses(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5)
    res, sizes = api.refine_wait(0)
    assert_scores_equal(mid_sc, alone_sc)
    assert np.array_equal(sizes, alone_sizes)
    assert res.tobytes() == alone_res.tobytes()


def test_private_context_gives_the_same_scores(gpu, model, scenario, hyps, noisy_scene):
    shared = api.score_poses(model, hyps, W, H, scenario["proj"], noisy_scene, 5)
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                box["sc"] = api.score_poses(model, hyps, W, H, scenario["proj"], noisy_scene, 5)
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert_scores_equal(box["sc"], shared)


def test_chunked_batch_matches_small_batches(gpu, model):
    """An 8192 x 2048 frame (2^24 pixels): a chunk of the depth workspace holds 64 hypotheses, so 150 span three chunks."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    poses = synth.hypotheses(150, seed=9)
    scene = api.render_host(model, synth.scene_pose()[None], Wb, Hb, proj)[0]
    rng = np.random.default_rng(2)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    whole = api.score_poses(model, poses, Wb, Hb, proj, sd, 4)
    parts = np.concatenate([api.score_poses(model, poses[i:i + 40], Wb, Hb, proj, sd, 4) for i in range(0, 150, 40)])
    assert_scores_equal(whole, parts)
    assert (whole["visible"] > 0).all() and whole["inlier"].sum() > 0


def test_batch_of_two_box_launches(gpu):
    """32768 + 5 hypotheses in one depth chunk: the launch over their boxes is split in two (grid.y is limited).  Every record is the
    reference's for its pose, the ones behind the split included; uint16 scene.  Behind the split every hypothesis takes the next pose
    (seam_cases.seam_index): a piece that read hypothesis j's pose or box for 32768 + j would give another record."""
    c = launch_split_case()
    idx = seam_index(c["P"], 8)
    got = api.score_poses(c["tris"], c["poses"][idx], c["W"], c["H"], c["proj"], c["scene"].astype(np.uint16), c["tau"])
    assert_seam_visible(c["scores"], idx)
    assert_records_take(got, c["scores"], idx)
