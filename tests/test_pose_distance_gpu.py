"""GPU tests (-m gpu) of pr_pose_distance: every field of every record equals the numpy reference of the header's definition
(tests/pose_dist_ref.py) bit for bit -- point counts around the kernel's chunk seams, pair counts around its 64-lane and 256-lane seams,
matrices, symmetry sets of every size, both template variants, points behind the camera, saturated terms, several launches per call --,
the clustering on a refined batch, and a call between pr_refine_submit and pr_refine_wait."""
import numpy as np
import pytest

import pose_dist_ref as R
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H

pytestmark = pytest.mark.gpu

K = synth.K_TEST
C = _lib.POSE_DIST_CHUNK


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(300)


@pytest.fixture(scope="module")
def gt():
    return synth.scene_pose()


@pytest.fixture(scope="module")
def verts(model):
    assert model.vertices.shape == (15736, 3)
    return model.vertices


@pytest.fixture(scope="module")
def syms7():
    return api.symmetry_rotations((0, 0, 1), 7)


def _same(got, want):
    assert got.dtype == _lib.POSE_DIST and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError((len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)], want[tuple(bad[:5].T)]))


def test_chunk_constant(gpu):
    assert api.get_option("pose_dist_chunk") == C and C >= 64


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1])
def test_point_counts(gpu, verts, hyps, syms7, n_points):
    pts = np.ascontiguousarray(verts[:n_points])
    a, b = hyps[1:6], hyps[6:11]
    _same(api.pose_distance(pts, a, b, syms7, K), R.pairs(pts, a, b, syms7, K))
    _same(api.pose_distance(pts, a, b, syms7), R.pairs(pts, a, b, syms7))


def test_all_vertices(gpu, model, verts, hyps, gt, syms7):
    """8 pairs on all 15 736 vertices: one workgroup column, the point range over 62 workgroup rows."""
    a, b = hyps[1:9], hyps[9:17]
    _same(api.pose_distance(model, a, b, syms7, K), R.pairs(verts, a, b, syms7, K))
    _same(api.pose_distance(model.device_vertices(), a, gt, None, None), R.pairs(verts, a, gt))
    assert model.device_vertices() is model.device_vertices() and model.device_vertices().size() == 3 * 15736


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 257])
def test_pair_counts(gpu, verts, hyps, n_pairs):
    pts = np.ascontiguousarray(verts[::53])                       # 297 points: two chunks
    a, b = hyps[:n_pairs], hyps[300 - n_pairs:]
    syms3 = api.symmetry_rotations((1, 0, 0), 3)                  # 3 candidates per pair: the pairs straddle wavefronts and workgroups
    _same(api.pose_distance(pts, a, b, syms3, K), R.pairs(pts, a, b, syms3, K))
    _same(api.pose_distance(pts, a, b), R.pairs(pts, a, b))


@pytest.mark.parametrize("shape", [(3, 5), (65, 67)])
def test_matrices(gpu, verts, hyps, shape):
    pts = np.ascontiguousarray(verts[:2000])
    a, b = hyps[:shape[0]], hyps[100:100 + shape[1]]
    got = api.pose_distance_matrix(pts, a, b, None, K)
    assert got.shape == shape
    _same(got, R.matrix(pts, a, b, None, K))


def test_one_ground_truth(gpu, verts, hyps, gt, syms7):
    pts = np.ascontiguousarray(verts[:700])
    a = hyps[:17]
    want = R.pairs(pts, a, gt, syms7, K)
    _same(api.pose_distance(pts, a, gt, syms7, K), want)
    _same(api.pose_distance(pts, a, gt[None], syms7, K), want)
    _same(api.pose_distance_matrix(pts, a, gt, syms7, K), want.reshape(17, 1))
    _same(api.pose_distance_matrix(pts, gt, a, syms7, K), R.matrix(pts, gt, a, syms7, K))


def test_matrix_diagonal_and_rows(gpu, verts, hyps, syms7):
    pts = np.ascontiguousarray(verts[:1000])
    a = hyps[:20]
    m = api.pose_distance_matrix(pts, a, None, syms7, K)
    assert m.shape == (20, 20)
    zero = np.zeros((), _lib.POSE_DIST)
    zero["n_points"] = 1000
    for i in range(20):
        assert m[i, i].tobytes() == zero.tobytes()                # no displacement at all, found at symmetry index 0
        _same(api.pose_distance(pts, np.repeat(a[i:i + 1], 20, 0), a, syms7, K), m[i])
    _same(m[:4], R.matrix(pts, a[:4], a, syms7, K))


@pytest.mark.parametrize("n_syms", [0, 1, 2, 7, 64])
def test_symmetry_counts(gpu, verts, hyps, gt, n_syms):
    pts = np.ascontiguousarray(verts[::31])                       # 508 points
    a = hyps[1:7]
    syms = api.symmetry_rotations((0, 0, 1), n_syms) if n_syms else None
    got = api.pose_distance(pts, a, gt, syms, K)
    _same(got, R.pairs(pts, a, gt, syms, K))
    if n_syms == 0:                                               # no symmetries == the identity alone
        _same(got, api.pose_distance(pts, a, gt, np.eye(4, dtype=np.float32)[None], K))
        _same(got, api.pose_distance(pts, a, gt, np.zeros((0, 4, 4), np.float32), K))


def test_repeated_transform_reports_the_lower_index(gpu, verts, hyps):
    pts = np.ascontiguousarray(verts[::31])
    s = api.symmetry_rotations((0, 0, 1), 5)
    syms = np.stack([s[2], s[0], s[0], s[3], s[0]])               # the identity, three times, never first
    a = hyps[1:9]
    got = api.pose_distance(pts, a, a, syms, K)
    _same(got, R.pairs(pts, a, a, syms, K))
    assert (got["sym_sum"] == 1).all() and (got["sym_disp"] == 1).all() and (got["sym_proj"] == 1).all()
    assert not got["disp_sum_q16"].any() and not got["max_disp_sq"].any() and not got["max_proj_sq"].any()


def _small_transforms(rng, n):
    """The identity and n - 1 small rigid motions (a few degrees, a few mm): candidates that are no symmetries, so the three measures disagree."""
    out = [np.eye(4)]
    for _ in range(n - 1):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = np.deg2rad(rng.uniform(1.0, 8.0))
        kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        m = np.eye(4)
        m[:3, :3] = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        m[:3, 3] = rng.normal(size=3) * 3.0
        out.append(m)
    return np.stack(out).astype(np.float32)


def test_three_minima_on_three_candidates(gpu, verts, hyps, gt):
    pts = np.ascontiguousarray(verts[::53])
    syms = _small_transforms(np.random.default_rng(77), 8)
    a = hyps[1:60]
    want = R.pairs(pts, a, gt, syms, K)
    apart = [i for i in range(len(a)) if len({int(want["sym_sum"][i]), int(want["sym_disp"][i]), int(want["sym_proj"][i])}) == 3]
    assert len(apart) >= 3, apart                                 # the case exists in the reference: the comparison below is not vacuous
    got = api.pose_distance(pts, a, gt, syms, K)
    _same(got, want)
    assert all(len({int(got["sym_sum"][i]), int(got["sym_disp"][i]), int(got["sym_proj"][i])}) == 3 for i in apart)


def test_projection_variants(gpu, verts, hyps, gt, syms7):
    """K = None (the kernel without divisions) changes nothing but the two projection fields."""
    pts = np.ascontiguousarray(verts[:900])
    a = hyps[1:40]
    with_k, without = api.pose_distance(pts, a, gt, syms7, K), api.pose_distance(pts, a, gt, syms7)
    assert not without["max_proj_sq"].any() and not without["sym_proj"].any()
    assert with_k["max_proj_sq"].all() and np.isfinite(with_k["max_proj_sq"]).all()
    stripped = with_k.copy()
    stripped["max_proj_sq"], stripped["sym_proj"] = 0, 0
    _same(without, stripped)
    _same(with_k, R.pairs(pts, a, gt, syms7, K))


def test_points_behind_the_camera(gpu, verts, gt):
    pts = np.ascontiguousarray(verts[:900])
    near = gt.copy()
    near[2, 3] = 10.0                                             # the camera inside the model: part of it at Z <= 0
    assert ((pts @ near[:3, :3].T)[:, 2] + 10.0 <= 0).any() and ((pts @ near[:3, :3].T)[:, 2] + 10.0 > 0).any()
    away = np.eye(4, dtype=np.float32)
    away[:3, 3] = (near[:3, :3].T @ np.array([0, 0, 400.0])).astype(np.float32)      # near * away: the same model 400 mm further out
    for syms, k_want in ((None, 0), (np.stack([np.eye(4, dtype=np.float32), away]), 1), (np.stack([away, np.eye(4, dtype=np.float32)]), 0)):
        got = api.pose_distance(pts, near, gt, syms, K)
        _same(got, R.pairs(pts, near, gt, syms, K))
        if syms is None:
            assert np.isposinf(got["max_proj_sq"][0]) and got["sym_proj"][0] == 0
        else:
            assert np.isfinite(got["max_proj_sq"][0]) and got["sym_proj"][0] == k_want
        assert np.isfinite(got["max_disp_sq"]).all()
    # the other pose behind the camera, and both
    _same(api.pose_distance(pts, gt, near, None, K), R.pairs(pts, gt, near, None, K))
    got = api.pose_distance(pts, np.stack([gt, near, near]), np.stack([near, near, gt]), None, K)
    assert np.isposinf(got["max_proj_sq"]).all()
    assert not api.pose_distance(pts, near, gt)["max_proj_sq"].any()


def test_saturation(gpu, verts, hyps):
    pts = np.ascontiguousarray(verts[:300])
    a = hyps[1:4]
    b = a.copy()
    b[:, 0, 3] += np.float32(2e7)
    for kk in (None, K):
        got = api.pose_distance(pts, a, b, None, kk)
        _same(got, R.pairs(pts, a, b, None, kk))
        assert (got["disp_sum_q16"] == 300 * (1 << 40)).all()


def test_several_launches(gpu, verts, hyps):
    """600 x 600 pairs are more candidates than one launch takes: the matrix equals its two halves, each one launch, and the reference where
    it is sampled -- around the seam too."""
    pts = np.ascontiguousarray(verts[::400])                      # 40 points
    rng = np.random.default_rng(5)
    a = np.concatenate([hyps, hyps])
    a[300:, :3, 3] += rng.normal(size=(300, 3)).astype(np.float32)
    m = api.pose_distance_matrix(pts, a, None, None, K)
    assert m.shape == (600, 600) and 600 * 600 > (1 << 18)
    _same(m[:300], api.pose_distance_matrix(pts, a[:300], a, None, K))
    _same(m[300:], api.pose_distance_matrix(pts, a[300:], a, None, K))
    seam = [(p // 600, p % 600) for p in range((1 << 18) - 3, (1 << 18) + 3)]
    for i, j in seam + [(int(i), int(j)) for i, j in rng.integers(0, 600, (60, 2))]:
        assert m[i, j].tobytes() == R.record(pts, a[i], a[j], None, K).tobytes(), (i, j)


def test_model_from_triangles(gpu, hyps, gt):
    tris = np.random.default_rng(3).normal(size=(37, 3, 3)).astype(np.float32) * 40
    m = api.Model(tris=tris)
    assert m.device_vertices().size() == 37 * 9                   # the corners as they are
    _same(api.pose_distance(m, hyps[:5], gt, None, K), R.pairs(tris.reshape(-1, 3), hyps[:5], gt, None, K))


@pytest.fixture(scope="module")
def refined(gpu, model, scenario, hyps, gscenes):
    res, _ = api.refine_batch(model, hyps[:64], W, H, scenario["proj"], scenario["K"], gscenes["proj"], api.ICPConvergenceCriteria(0.0, 0.0, 20))
    return api.refined_poses(res, hyps[:64])


def test_refined_batch_end_to_end(gpu, model, verts, scenario, gt, refined):
    """Equality with the reference only; what the distances ARE is what tools/pose_accuracy.py records."""
    got = api.pose_distance(model, refined, gt, None, K)
    _same(got, R.pairs(verts, refined, gt, None, K))
    scores = api.score_poses(model, refined, W, H, scenario["proj"], scenario["depth"][1], 5)
    order = api.rank_hypotheses(scores)
    dist = api.pose_distance_matrix(model, refined)
    for radius in (0.05, 1.0, 20.0):
        kept, rep = api.merge_duplicates(order, dist, radius)
        want_kept, want_rep = R.cluster_greedy(order, dist, radius)
        assert kept.tolist() == want_kept and rep.tolist() == want_rep.tolist()
        assert kept[0] == order[0] and 1 <= len(kept) <= 64
    print("mean displacement of 64 refined hypotheses: median %.4f mm, max %.3f mm; distinct at 1 mm: %d" %
          (np.median(api.mean_displacement(got)), api.mean_displacement(got).max(), len(api.merge_duplicates(order, dist, 1.0)[0])))


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_call_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, refined, syms7, solve):
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
        alone_res, alone_sizes = api.refine_batch(model, hyps[:256], W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        alone = api.pose_distance_matrix(model, refined, None, syms7, K)
        api.refine_submit(0, model, hyps[:256], W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        mid = api.pose_distance_matrix(model, refined, None, syms7, K)
        res, sizes = api.refine_wait(0)
        _same(mid, alone)
        assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()
    finally:
        api.set_option("solve", before)
