"""GPU tests (-m gpu) of pr_pose_vsd / pr_pose_vsd_multi: every record is held byte for byte to the numpy float32 restatement of the header's
definition (tests/vsd_ref.py) over the oracle's renders -- both scene types, with and without K, every number of taus, pixel boxes of every
relative position, one truth for many estimates, the launch and chunk seams, a realistic frame, mixed batches and a pending slot."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import vsd_ref as R
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import assert_records_repeat

pytestmark = pytest.mark.gpu

TAUS12 = R.SMALL_TAUS + (88.0, 96.0)
DIAMETER = 154.5                                                    # obj_06, mm
TAUS_BOP_MM = tuple(np.float32(t * DIAMETER) for t in api.VSD_TAUS_BOP)


def _same(got, want):
    R.assert_vsd_equal(got, want)


# ---- the 32-pair small case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("with_k", [True, False])
@pytest.mark.parametrize("n_taus", [0, 1, 10, 12])
def test_small_case(gpu, dtype, with_k, n_taus):
    c = R.small_case()
    scene = np.ascontiguousarray(c["scene"].astype(dtype))
    K, taus = (c["K"] if with_k else None), TAUS12[:n_taus]
    got = api.pose_vsd(c["tris"], c["est"], c["gt"], c["W"], c["H"], c["proj"], scene, K, c["delta"], taus)
    want = R.vsd_ref(c["r_est"], c["r_gt"], scene, K, c["delta"], taus)
    _same(got, want)
    assert (got["far"][:, n_taus:] == 0).all() and got["inter"].min() > 0
    if not with_k:
        _same(got, R.vsd_int(c["r_est"], c["r_gt"], scene, 15, [int(t) for t in taus]))
    if n_taus:
        assert got["far"][:, 0].max() >= 100


def test_estimate_equal_to_truth(gpu):
    c = R.small_case()
    got = api.pose_vsd(c["tris"], c["gt"], c["gt"], c["W"], c["H"], c["proj"], c["scene"], c["K"], c["delta"], [0.0, 1.0, 8.0])
    _same(got, R.vsd_ref(c["r_gt"], c["r_gt"], c["scene"], c["K"], c["delta"], [0.0, 1.0, 8.0]))
    for f in ("uni", "visib_gt", "visib_est"):
        assert np.array_equal(got[f], got["inter"]), f
    assert (got["inter"] > 0).all() and np.array_equal(got["far"][:, 0], got["inter"]) and not got["far"][:, 1:].any()
    assert not api.vsd_errors(got, 3)[:, 1:].any() and (api.vsd_errors(got, 3)[:, 0] == 1.0).all()


# ---- box geometry: a 600 x 40 frame (three row blocks: 16, 16, 8; more than two column steps) ----------------------------------------------
GW, GH = 600, 40
GK = np.array([300.0, 0, 299.5, 0, 300.0, 19.5, 0, 0, 1], np.float32)


def _at(x, y, z, angles=(0.0, 0.0, 0.0)):
    return synth.pose_matrix(synth.euler_zyx(angles), np.array([x, y, z], np.float32))


@functools.lru_cache(maxsize=None)
def geometry_case():
    proj = api.compute_proj(GK, GW, GH)
    rng = np.random.default_rng(3)
    scene = (395 + rng.integers(-30, 31, (GH, GW))).astype(np.int64)      # a noisy plane about where the boxes' front faces are
    scene[rng.random(scene.shape) < 0.15] = 0
    scene[rng.random(scene.shape) < 0.15] = 900
    scene[rng.random(scene.shape) < 0.05] = 120
    return dict(proj=proj, scene=scene.astype(np.int32))


def _geometry(tris, est, gt):
    c = geometry_case()
    est, gt = np.stack(est), np.stack(gt)
    r_est, r_gt = O.render(tris, est, GW, GH, c["proj"]), O.render(tris, gt, GW, GH, c["proj"])
    for dt in (np.int32, np.uint16):
        scene = np.ascontiguousarray(c["scene"].astype(dt))
        got = api.pose_vsd(tris, est, gt, GW, GH, c["proj"], scene, GK, 15.0, R.SMALL_TAUS)
        _same(got, R.vsd_ref(r_est, r_gt, scene, GK, 15.0, R.SMALL_TAUS))
    return got, r_est > 0, r_gt > 0


def _cols(mask):
    return np.flatnonzero(mask.any(0))


def _rows(mask):
    return np.flatnonzero(mask.any(1))


def test_box_wider_than_the_column_step(gpu):
    got, me, mg = _geometry(R.box_mesh((200, 8, 8)), [_at(0, -3, 400, (0.02, 0.0, 0.01))], [_at(10, 3, 400)])
    assert len(_cols(me[0])) > 256 and len(_cols(mg[0])) > 256 and _cols(me[0] | mg[0])[-1] - _cols(me[0] | mg[0])[0] > 512 - 256
    assert got["inter"][0] > 0 and got["inter"][0] < got["uni"][0]


def test_boxes_in_every_relative_position(gpu):
    far_off = _at(1.0e5, 0, 400)
    a, b = _at(-20, -6, 400, (0.1, 0.05, 0.0)), _at(0, 6, 400)        # a's box starts left of and above (or below) b's and ends inside it
    est = [a, b, _at(-150, 0, 400), far_off, _at(5, 2, 400), far_off]
    gt = [b, a, _at(150, 0, 400), _at(5, 2, 400), far_off, far_off]
    got, me, mg = _geometry(R.box_mesh((30, 14, 10)), est, gt)
    # pairs 0 and 1: the union spans both row-block boundaries; each box starts outside the other and ends inside it, and the mirror image
    u = me[0] | mg[0]
    assert _rows(u)[0] < 16 and _rows(u)[-1] >= 32
    assert _cols(me[0])[0] < _cols(mg[0])[0] <= _cols(me[0])[-1] < _cols(mg[0])[-1]
    assert (_rows(me[0])[0] < _rows(mg[0])[0] <= _rows(me[0])[-1] < _rows(mg[0])[-1]) or (_rows(mg[0])[0] < _rows(me[0])[0] <= _rows(mg[0])[-1] < _rows(me[0])[-1])
    assert got["inter"][0] > 0 and got["inter"][1] > 0 and got["uni"][0] == got["uni"][1]      # (vg || ve is symmetric in the two poses; vg && ve is not)
    # pair 2: disjoint boxes
    assert not (me[2] & mg[2]).any() and _cols(me[2])[-1] < _cols(mg[2])[0]
    assert got["inter"][2] == 0 and got["uni"][2] == got["visib_gt"][2] + got["visib_est"][2] and got["visib_gt"][2] > 0 and got["visib_est"][2] > 0
    assert not got["far"][2].any()
    # pairs 3, 4, 5: the estimate renders nothing, the truth renders nothing, neither does
    assert not me[3].any() and got["visib_est"][3] == 0 and got["uni"][3] == got["visib_gt"][3] > 0 and got["inter"][3] == 0
    assert not mg[4].any() and got["visib_gt"][4] == 0 and got["uni"][4] == got["visib_est"][4] > 0 and got["inter"][4] == 0
    assert got[5].tobytes() == bytes(64)
    assert np.array_equal(api.vsd_errors(got, 10)[3:], np.ones((3, 10)))


def test_boxes_touch_all_four_frame_borders(gpu):
    got, me, mg = _geometry(R.box_mesh((700, 60, 10)), [_at(3, 1, 390, (0.01, 0.02, 0.0))], [_at(0, 0, 400)])
    for m in (me[0], mg[0]):
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    assert got["uni"][0] > 0.5 * GW * GH and got["far"][0][0] > 0


# ---- one truth, seams ---------------------------------------------------------------------------------------------------------------------
def test_one_truth_for_many_estimates(gpu):
    c = R.small_case()
    est, gt = c["est"][:17], c["gt"][5]
    pairs = api.pose_vsd(c["tris"], est, np.repeat(gt[None], 17, 0), c["W"], c["H"], c["proj"], c["scene"], c["K"], c["delta"], c["taus"])
    _same(pairs, R.vsd_ref(c["r_est"][:17], c["r_gt"][5], c["scene"], c["K"], c["delta"], c["taus"]))
    for one in (gt, gt[None]):
        assert api.pose_vsd(c["tris"], est, one, c["W"], c["H"], c["proj"], c["scene"], c["K"], c["delta"], c["taus"]).tobytes() == pairs.tobytes()
    assert api.pose_vsd(c["tris"], est[:1], gt, c["W"], c["H"], c["proj"], c["scene"], c["K"], c["delta"], c["taus"]).tobytes() == pairs[:1].tobytes()


def test_batch_of_two_launches(gpu):
    """32768 + 5 pairs in one depth chunk: the launch over the pairs is split in two (grid.y is limited); uint16 scene.  Behind the split every
    pair is the next of the 32 (seam_cases.seam_index), so pair 32768 + j never expects pair j's record."""
    c = R.small_case()
    want = R.vsd_ref(c["r_est"], c["r_gt"], c["scene"], c["K"], c["delta"], c["taus"])
    idx = seam_index(32768 + 5, 32)
    assert_seam_visible(want, idx)
    got = api.pose_vsd(c["tris"], c["est"][idx], c["gt"][idx], c["W"], c["H"], c["proj"], c["scene"].astype(np.uint16), c["K"], c["delta"], c["taus"])
    assert_records_take(got, want, idx)


def test_chunked_batch(gpu):
    """A 2048 x 2048 frame: a chunk of the depth workspace holds 256 renders, so 300 pairs (600 renders) span three chunks, and 300 estimates
    against one truth two (each with its own render of the truth); 129 estimates against one truth fit one."""
    Wb = Hb = 2048
    K = np.array([1200.0, 0, 1023.5, 0, 1200.0, 1023.5, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    tris = R.box_mesh()
    rng = np.random.default_rng(8)
    gt = np.stack([_at(40.0 * i - 80, 25.0 * i - 60, 380 + 10 * i, (0.3 * i, 0.5 - 0.2 * i, 0.1 * i)) for i in range(5)])
    est = np.stack([R.perturbed(g, rng, 0.05, 6.0) for g in gt])
    r_est, r_gt = O.render(tris, est, Wb, Hb, proj), O.render(tris, gt, Wb, Hb, proj)
    front = np.where(r_gt[:3] > 0, r_gt[:3], 2**31 - 1).min(0)
    front[front == 2**31 - 1] = 0
    scene = np.where(rng.random(front.shape) < 0.1, 0, front + rng.integers(-12, 13, front.shape) * (front > 0))
    scene[(front == 0) & (rng.random(front.shape) < 0.5)] = 800
    scene = scene.astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    taus = R.SMALL_TAUS[:4]
    want = R.vsd_ref(r_est, r_gt, scene, K, 15.0, taus)
    assert (want["inter"] > 0).all() and want["far"][:, 0].min() > 0
    idx = np.arange(300) % 5
    assert_records_repeat(api.pose_vsd(tris, est[idx], gt[idx], Wb, Hb, proj, sd, K, 15.0, taus), want)
    one = R.vsd_ref(r_est, r_gt[0], scene, K, 15.0, taus)
    assert_records_repeat(api.pose_vsd(tris, est[idx[:129]], gt[0], Wb, Hb, proj, sd, K, 15.0, taus), one)
    assert_records_repeat(api.pose_vsd(tris, est[idx], gt[0], Wb, Hb, proj, sd, K, 15.0, taus), one)


# ---- realistic size -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy_scene(scenario):
    """test_verify_gpu.py's recipe: depth[1] with holes (0), +-k mm perturbations and background in front of / behind where a hypothesis may render."""
    rng = np.random.default_rng(20)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    bg = d == 0
    d[bg & (rng.random(d.shape) < 0.5)] = 900
    d[bg & (rng.random(d.shape) < 0.1)] = 150
    d[rng.random(d.shape) < 0.08] = 0
    return d.astype(np.int32)


@pytest.fixture(scope="module")
def realistic(scenario):
    est, gt = synth.hypotheses(64), synth.scene_pose()
    return est, gt, O.render(scenario["tris"], est, W, H, scenario["proj"]), O.render(scenario["tris"], gt[None], W, H, scenario["proj"])[0]


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
def test_realistic_frame(gpu, model, scenario, noisy_scene, realistic, dtype):
    est, gt, r_est, r_gt = realistic
    scene = np.ascontiguousarray(noisy_scene.astype(dtype))
    got = api.pose_vsd(model, est, gt, W, H, scenario["proj"], api.DeviceVector.from_host(scene.reshape(-1)), synth.K_TEST, api.VSD_DELTA_BOP, TAUS_BOP_MM)
    _same(got, R.vsd_ref(r_est, r_gt, scene, synth.K_TEST, api.VSD_DELTA_BOP, TAUS_BOP_MM))
    assert (got["inter"] > 0).all() and (got["inter"] < got["uni"]).any() and got["far"][:, 0].max() > 0
    e = api.vsd_errors(got, 10)
    assert e.shape == (64, 10) and (e >= 0).all() and (e <= 1).all() and 0.0 <= api.vsd_recall(e) <= 1.0


# ---- mixed batches ------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_single_mesh_calls(gpu, scenario, noisy_scene):
    meshes = [R.box_mesh(), np.ascontiguousarray(R.box_mesh() * np.float32(0.6)), np.ascontiguousarray(scenario["tris"][:2000])]
    rng = np.random.default_rng(4)
    idx = rng.permutation(np.repeat(np.arange(3), 5))
    gt = synth.hypotheses(16)[1:]
    est = np.stack([R.perturbed(g, rng, 0.04, 5.0) for g in gt])
    args = (W, H, scenario["proj"], api.DeviceVector.from_host(noisy_scene.reshape(-1)), synth.K_TEST, 15.0, TAUS_BOP_MM)
    got = api.pose_vsd_multi(meshes, idx, est, gt, *args)
    for m in range(3):
        sel = np.flatnonzero(idx == m)
        assert got[sel].tobytes() == api.pose_vsd(meshes[m], est[sel], gt[sel], *args).tobytes(), m
        _same(got[sel], R.vsd_ref(O.render(meshes[m], est[sel], W, H, scenario["proj"]), O.render(meshes[m], gt[sel], W, H, scenario["proj"]), noisy_scene,
                                  synth.K_TEST, 15.0, TAUS_BOP_MM))
    assert (got["uni"] > 0).all()
    # an empty mesh renders nothing: its pairs are all zero, the others keep their bytes
    with_empty = meshes + [np.zeros((0, 3, 3), np.float32)]
    idx2 = idx.copy()
    idx2[[2, 9]] = 3
    got2 = api.pose_vsd_multi(with_empty, idx2, est, gt, *args)
    keep = np.flatnonzero(idx2 != 3)
    assert got2[keep].tobytes() == got[keep].tobytes() and got2[[2, 9]].tobytes() == bytes(128)
    assert api.pose_vsd(np.zeros((0, 3, 3), np.float32), est[:3], gt[:3], *args).tobytes() == bytes(192)
    # a mesh index out of range: PR_ERR_INVALID, nothing written
    table, devs = api._mesh_table(meshes)
    bad = np.ascontiguousarray(idx, np.uint32)
    bad[7] = 3
    e32, g32, pj, taus = (np.ascontiguousarray(a, np.float32) for a in (est, gt, scenario["proj"], TAUS_BOP_MM))
    out = np.full(15 * 64, 0xAB, np.uint8)
    rc = _lib.load().pr_pose_vsd_multi(table, 3, bad.ctypes.data, e32.ctypes.data, 15, g32.ctypes.data, 15, W, H, pj.ctypes.data, args[3].data(), 1,
                                       synth.K_TEST.ctypes.data, 15.0, taus.ctypes.data, len(taus), out.ctypes.data)
    assert rc == _lib.PR_ERR_INVALID and (out == 0xAB).all()
    with pytest.raises(ValueError):
        api.pose_vsd_multi(meshes, bad, est, gt, *args)


# ---- a batch pending on a slot ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_vsd_between_submit_and_wait(gpu, model, scenario, gscenes, noisy_scene, realistic, solve):
    """A synchronous VSD call while a batch is pending on a slot of the same context: both give what they give alone."""
    est, gt, _, _ = realistic
    hyps = synth.hypotheses(256)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    vsd = lambda: api.pose_vsd(model, est, gt, W, H, scenario["proj"], noisy_scene, synth.K_TEST, api.VSD_DELTA_BOP, TAUS_BOP_MM)  # noqa: E731
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        alone = vsd()
        api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        mid = vsd()
        res, sizes = api.refine_wait(0)
    finally:
        api.set_option("solve", before)
    assert mid.tobytes() == alone.tobytes() and alone["inter"].min() > 0
    assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()
