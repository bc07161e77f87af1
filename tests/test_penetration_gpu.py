"""The span render and the pairwise interpenetration records on the device against tests/solid_ref.py (pinned to the oracle by
test_penetration_host.py): every plane and every field of every record, bit for bit."""
import numpy as np
import pytest

import oracle_lib as O
from gpu_common import W, H, pathological_hypotheses, random_mesh, random_pose
from pose_refine_amd import api, synth
from solid_ref import (PLANTED_KEPT, box_mesh, check_invariants, pairs_ref, planted, shifted, span_ref, span_ref_multi)

pytestmark = pytest.mark.gpu


def _span(model, poses, w, h, proj, roi=(0, 0, 0, 0)):
    near, far = api.render_span(model, poses, w, h, proj, roi)
    shape = (len(poses), roi[3], roi[2]) if roi[2] > 0 and roi[3] > 0 else (len(poses), h, w)
    assert near.to_host().tobytes() == api.render(model, poses, w, h, proj, roi).to_host().tobytes()
    return near.to_host().reshape(shape), far.to_host().reshape(shape)


def _assert_pairs(got, want):
    assert got.dtype == api.PAIR_SOLID and got.shape == want.shape
    for f in api.PAIR_SOLID.names:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (f, bad[:5].tolist(), [(int(got[f][i, j]), int(want[f][i, j])) for i, j in bad[:5]])
    assert got.tobytes() == want.tobytes()
    check_invariants(got)


# ---- render_span -----------------------------------------------------------------------------------------------------------------------
def test_span_full_frame(gpu, model, scenario):
    poses = synth.hypotheses(24)
    near, far = _span(model, poses, W, H, scenario["proj"])
    ref_near, ref_far = span_ref(scenario["tris"], poses, scenario["proj"], W, H)
    assert np.array_equal(near, ref_near) and np.array_equal(far, ref_far)
    assert (far > near).sum() > 24 * 5000


def test_span_odd_frame(gpu, model, scenario):
    w, h = 333, 251
    K = np.array([300.0, 0, 166.3, 0, 300.0, 124.8, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, w, h)
    poses = synth.hypotheses(7)
    near, far = _span(model, poses, w, h, proj)
    ref_near, ref_far = span_ref(scenario["tris"], poses, proj, w, h)
    assert np.array_equal(near, ref_near) and np.array_equal(far, ref_far) and (far > near).sum() > 7 * 1000


@pytest.mark.parametrize("roi", [(200, 150, 200, 180), (0, 100, 330, 200), (100, 0, 300, 240)])
def test_span_roi(gpu, model, scenario, roi):
    poses = synth.hypotheses(6)
    near, far = _span(model, poses, W, H, scenario["proj"], roi)
    ref_near, ref_far = span_ref(scenario["tris"], poses, scenario["proj"], W, H, roi)
    assert np.array_equal(near, ref_near) and np.array_equal(far, ref_far) and far.any()


def test_span_pathological_hypotheses(gpu, model, scenario):
    """NaN / infinite / zero matrices, the camera inside the object, behind it, a giant, a speck, good poses between them.  A small frame: the giant's
    triangles each cover all of it, and the reference walks every candidate pixel."""
    w, h = 160, 120
    K = np.array([143.0, 0, 81.3, 0, 143.0, 60.5, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, w, h)
    bad, idx_bad = pathological_hypotheses(synth.hypotheses(24))
    near, far = _span(model, bad, w, h, proj)
    ref_near, ref_far = span_ref(scenario["tris"], bad, proj, w, h)
    for i in range(24):
        assert np.array_equal(near[i], ref_near[i]) and np.array_equal(far[i], ref_far[i]), i
    good = [i for i in range(24) if i not in idx_bad]
    assert all((far[i] > near[i]).sum() > 300 for i in good) and sum(bool(far[i].any()) for i in idx_bad) >= 4


def test_span_random_mesh_and_empty_mesh(gpu, scenario):
    rng = np.random.default_rng(31)
    w, h = 97, 61
    K = np.array([1.1 * w, 0, w / 2 + 3.3, 0, 1.2 * w, h / 2 - 2.1, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, w, h)
    tris = random_mesh(rng, 400, 40.0)                               # degenerate and duplicate triangles among them
    poses = np.stack([random_pose(rng, d) for d in (300.0, 150.0, 90.0, 600.0, 45.0)])
    poses[4, 2, 3] = 10.0                                           # the camera inside the soup
    m = api.Model(tris=tris)
    for roi in ((0, 0, 0, 0), (11, 7, 50, 40)):
        near, far = _span(m, poses, w, h, proj, roi)
        ref_near, ref_far = span_ref(tris, poses, proj, w, h, roi)
        assert np.array_equal(near, ref_near) and np.array_equal(far, ref_far)
    assert np.array_equal(ref_near, O.render(tris, poses, w, h, proj, roi))
    none = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    near, far = _span(none, poses, w, h, proj)
    assert not near.any() and not far.any()
    assert not api.pose_penetration(none, poses, w, h, proj).view(np.uint8).any()
    with pytest.raises(api.PoseRefineError):
        api.check(api._lib.load().pr_render_span(m.device_tris().data(), len(tris), api.ptr(api._f32(poses, (-1, 16))), 5, w, h, api.ptr(api._f32(proj, -1)),
                                                 api.Roi(0, 0, 0, 0), api.DeviceVector(5 * w * h, np.int32).data(), None))


# ---- pose_penetration --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ten(scenario):
    """The planted five, four seeded hypotheses and S far away; their reference planes."""
    poses = np.concatenate([planted(), synth.hypotheses(8)[:4], shifted(synth.scene_pose(), 30, -20, 700)[None]])
    return poses, span_ref(scenario["tris"], poses, scenario["proj"], W, H, raw=True)


@pytest.mark.parametrize("slack", [0, 2, 50])
def test_pairs_of_the_ten_poses(gpu, model, scenario, ten, slack):
    poses, (near, far) = ten
    got = api.pose_penetration(model, poses, W, H, scenario["proj"], slack)
    _assert_pairs(got, pairs_ref(near, far, slack))
    assert got["both"][0, 2] > 10000 and got["inter"][0, 2] == 0     # behind S: thousands of shared pixels, no shared volume
    if slack == 0:
        assert np.round(api.penetration_fraction(got)[0, :5], 3).tolist() == [1.0, 0.760, 0.0, 0.0, 0.470]


@pytest.fixture(scope="module")
def thirty_three(scenario):
    poses = synth.hypotheses(33)
    return poses, span_ref(scenario["tris"], poses, scenario["proj"], W, H, raw=True)


@pytest.mark.parametrize("P", [5, 6, 33])
def test_pair_ownership_odd_and_even(gpu, model, scenario, thirty_three, P):
    """Every unordered pair has one owner: P odd, P even (the distance P / 2 belongs to the lower index) and more partners than wavefronts."""
    poses, (near, far) = thirty_three
    got = api.pose_penetration(model, poses[:P], W, H, scenario["proj"], 0)
    _assert_pairs(got, pairs_ref(near[:P], far[:P], 0))
    assert (got["inter"] > 0).all()                                  # hypotheses about one pose: every pair interpenetrates
    # a second call, and the batch reversed: the same bytes, permuted
    assert api.pose_penetration(model, poses[:P], W, H, scenario["proj"], 0).tobytes() == got.tobytes()
    rev = api.pose_penetration(model, poses[:P][::-1], W, H, scenario["proj"], 0)
    assert np.ascontiguousarray(rev[::-1, ::-1]).tobytes() == got.tobytes()


def test_boxes_bands_edges_and_empty_rows(gpu, model, scenario):
    """Two identical poses; one off screen; one at z = 120 mm whose box is the frame (many LDS bands) beside small far ones whose boxes fit one band;
    boxes cut by each of the four frame edges."""
    S = synth.scene_pose()
    near_pose = S.copy(); near_pose[:3, 3] = [0, 0, 120]
    poses = np.stack([S, S, shifted(S, 3000, 0, 0), near_pose, shifted(S, 0, 0, 900), shifted(S, 12, 8, 930),
                      shifted(S, -190, 0, 0), shifted(S, 150, 0, 0), shifted(S, 0, -140, 0), shifted(S, 0, 110, 0)])
    near, far = span_ref(scenario["tris"], poses, scenario["proj"], W, H, raw=True)
    drawn = (near != np.iinfo(np.int32).max) & (near > 0)
    assert not drawn[2].any() and drawn[3].sum() > 100000           # off screen; most of the frame
    assert 0 < drawn[4].sum() < 3000 and (drawn[4] & drawn[5]).any()   # small enough for one band (8192 pixels), and they meet
    assert drawn[6][:, 0].any() and drawn[7][:, -1].any() and drawn[8][0].any() and drawn[9][-1].any()      # cut by the left, right, top and bottom edge
    want = pairs_ref(near, far, 0)
    got = api.pose_penetration(model, poses, W, H, scenario["proj"], 0)
    _assert_pairs(got, want)
    assert got[0, 1] == got[0, 0] == got[1, 1] and got["sum_mm"][0, 0] > 0      # identical poses: the off-diagonal record is the diagonal's
    assert not got[2].view(np.uint8).any() and not got[:, 2].copy().view(np.uint8).any()      # off screen: a row and a column of zeros
    assert got["both"][3, 0] > 0 and got["inter"][3, 3] > 100000 and got["inter"][4, 5] > 0
    assert api.pose_penetration(model, poses, W, H, scenario["proj"], 0).tobytes() == got.tobytes()
    rev = api.pose_penetration(model, poses[::-1], W, H, scenario["proj"], 0)
    assert np.ascontiguousarray(rev[::-1, ::-1]).tobytes() == got.tobytes()
    _assert_pairs(api.pose_penetration(model, poses, W, H, scenario["proj"], 7), pairs_ref(near, far, 7))


# ---- mixed batches -----------------------------------------------------------------------------------------------------------------------
def test_mixed_batch(gpu, model, scenario):
    S = synth.scene_pose()
    meshes = [scenario["tris"], box_mesh(40, 30, 25), synth.uv_sphere_mesh(24, 12)]
    idx = np.array([2, 0, 1, 1, 0, 2, 0, 1, 2], np.uint32)           # interleaved in the caller's order
    poses = np.stack([shifted(S, 10 * k - 40, 6 * (k % 3) - 6, 15 * (k % 4)) for k in range(9)])
    near, far = span_ref_multi(meshes, idx, poses, scenario["proj"], W, H)
    for slack in (0, 5):
        got = api.pose_penetration_multi(meshes, idx, poses, W, H, scenario["proj"], slack)
        _assert_pairs(got, pairs_ref(near, far, slack))
    assert (got["inter"] > 0).sum() > 40                             # meshes of different kinds do meet
    # one mesh through the mixed entry point: the single-mesh call's bytes
    one = api.pose_penetration_multi([model], np.zeros(9, np.uint32), poses, W, H, scenario["proj"], 0)
    assert one.tobytes() == api.pose_penetration(model, poses, W, H, scenario["proj"], 0).tobytes()
    with pytest.raises(ValueError):
        api.pose_penetration_multi(meshes, [0, 1, 3], poses[:3], W, H, scenario["proj"])


def test_mixed_batch_empty_and_unused_meshes(gpu, scenario):
    """The frame, K, soup and poses of test_span_random_mesh_and_empty_mesh as a mixed batch whose table holds an empty mesh with hypotheses and a mesh
    with none; then every hypothesis on the empty mesh: no raster launches, yet both planes must be filled -- the workspaces still hold the first
    call's renders -- so that every byte of every record is zero."""
    rng = np.random.default_rng(31)
    w, h = 97, 61
    K = np.array([1.1 * w, 0, w / 2 + 3.3, 0, 1.2 * w, h / 2 - 2.1, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, w, h)
    tris = random_mesh(rng, 400, 40.0)
    poses = np.stack([random_pose(rng, d) for d in (300.0, 150.0, 90.0, 600.0, 45.0)])
    poses[4, 2, 3] = 10.0
    meshes = [tris, np.zeros((0, 3, 3), np.float32), box_mesh(40, 30, 25), synth.uv_sphere_mesh(24, 12)]      # the sphere gets no hypothesis
    idx = np.array([0, 1, 2, 0, 1], np.uint32)
    near, far = span_ref_multi(meshes, idx, poses, proj, w, h)
    for slack in (0, 5):
        _assert_pairs(api.pose_penetration_multi(meshes, idx, poses, w, h, proj, slack), pairs_ref(near, far, slack))
    got = api.pose_penetration_multi(meshes, np.ones(5, np.uint32), poses, w, h, proj, 0)
    assert got.shape == (5, 5) and not got.view(np.uint8).any()


# ---- the planted frame end to end ------------------------------------------------------------------------------------------------------------
def test_planted_frame_end_to_end(gpu, model, scenario):
    scene = scenario["depth"][1]
    poses = planted()
    before = api.score_poses(model, poses, W, H, scenario["proj"], scene, 10)
    pairs = api.pose_penetration(model, poses, W, H, scenario["proj"])
    assert api.select_disjoint(np.arange(5), pairs).tolist() == PLANTED_KEPT
    assert api.score_poses(model, poses, W, H, scenario["proj"], scene, 10).tobytes() == before.tobytes()      # the existing calls are undisturbed
    assert before["inlier"][0] > 10000
