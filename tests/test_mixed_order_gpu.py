"""GPU tests (-m gpu) of a mixed batch's way back to the caller's order: a wrong index in a gather or a scatter of the entry-point layer.
Five hypotheses of three tiny meshes (the middle one unused) in a 64 x 48 frame.  Every per-hypothesis output of a mixed call equals, byte
for byte, the single-mesh call on that mesh's hypotheses, placed at the caller's indices; the outputs that relate hypotheses of different
meshes (the overlap matrix, the penetration records, the cover walk, the composition) and the full-frame renders are held to the same call
with poses and mesh index permuted together.  The hypotheses lie at distinct depths with depth ranges that do not meet, so no pixel has two
renders at one depth and no result depends on which hypothesis comes first."""
import numpy as np
import pytest

from pose_refine_amd import api, synth

pytestmark = pytest.mark.gpu

W, H = 64, 48
K = np.array([120.0, 0.0, 32.0, 0.0, 120.0, 24.0, 0.0, 0.0, 1.0], np.float32)
IDX = np.array([2, 0, 2, 0, 2])
PI = np.array([3, 0, 4, 1, 2])                                     # hypothesis k of the permuted call is hypothesis PI[k] of the original
TAU_ALL = 2000                                                     # every rendered pixel is an inlier of the scene: cross-mesh overlaps are not 0
CRIT = api.ICPConvergenceCriteria(0.0, 0.0, 3)


def _box(s):
    """The 12 triangles of the cube [-s, s]^3."""
    c = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.ascontiguousarray([[c[a], c[b], c[d]] for q in quads for a, b, d in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.float32)


@pytest.fixture(scope="module")
def kit(gpu):
    meshes = [_box(20.0), _box(30.0), _box(40.0)]
    half = [20.0, 30.0, 40.0]
    depth = [560.0, 260.0, 700.0, 340.0, 860.0]                  # with the boxes' rotated half-diagonals (< 1.5 s) the depth ranges do not meet
    pixel = [(0, 6), (-6, 2), (4, -5), (-4, -5), (6, 2)]         # the centres on a ring around the principal point: every two silhouettes overlap, none is hidden
    poses = np.stack([synth.pose_matrix(synth.euler_zyx((0.10 + 0.03 * i, -0.15 + 0.05 * i, 0.2 * i)),
                                        np.array([pixel[i][0] * depth[i] / 120.0, pixel[i][1] * depth[i] / 120.0, depth[i]], np.float32)) for i in range(5)])
    proj = api.compute_proj(K, W, H)
    for i in range(5):
        assert 1.5 * half[IDX[i]] < min(abs(depth[i] - depth[j]) - 1.5 * half[IDX[j]] for j in range(5) if j != i)
    # the scene: the five objects 3 mm behind their hypotheses in front of a wall, every pixel measured
    moved = poses.copy()
    moved[:, 2, 3] += 3.0
    shots = np.stack([api.render_host(meshes[IDX[i]], moved[i:i + 1], W, H, proj)[0] for i in range(5)])
    assert all((shots[i] > 0).sum() > 60 for i in range(5))
    front = np.where(shots > 0, shots, 1 << 30).min(0)
    for i in range(5):
        assert ((shots[i] == front) & (shots[i] > 0)).sum() >= 8, i           # a part of every object is the scene's surface
        for j in range(i):
            assert ((shots[i] > 0) & (shots[j] > 0)).any(), (i, j)
    scene = np.where(shots > 0, shots, 1000).min(0).astype(np.int32)
    return dict(meshes=meshes, poses=poses, proj=proj, scene=scene, sd=api.DeviceVector.from_host(scene.reshape(-1)),
                icp=api.Scene_projective().init_Scene_projective_cuda(scene, K, W, H),
                centers=np.zeros((3, 3), np.float32), radii=np.array([h * np.sqrt(3.0) / 1000.0 for h in half], np.float32))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _per_mesh(kit, multi, single, n_out, axis=None):
    """multi(meshes, idx, poses) against single(mesh, poses[sel], m) per mesh: output k of the mixed call, taken at the mesh's hypotheses, is the single call's."""
    got = multi(kit["meshes"], IDX, kit["poses"])
    assert len(got) == n_out
    for m in (0, 2):
        sel = np.flatnonzero(IDX == m)
        want = single(kit["meshes"][m], kit["poses"][sel], m)
        for k in range(n_out):
            g = got[k][:, sel] if axis and axis[k] == 1 else got[k][sel]
            assert _same(np.ascontiguousarray(g), np.ascontiguousarray(want[k])), (m, k)
    return got


# ---- per-mesh equality -------------------------------------------------------------------------------------------------------------------
def test_refine_batch(kit):
    args = (W, H, kit["proj"], K, kit["icp"], CRIT)
    res, sizes = _per_mesh(kit, lambda ms, ix, p: api.refine_batch_multi(ms, ix, p, *args), lambda t, p, m: api.refine_batch(t, p, *args), 2)
    assert (sizes > 0).all() and len(set(sizes.tolist())) == 5


def test_refine_pyramid_levels(kit):
    args = (W, H, kit["proj"], K, kit["icp"])
    levels = [(2, CRIT), (1, CRIT)]
    res, lres, lsizes = _per_mesh(kit, lambda ms, ix, p: api.refine_pyramid_multi(ms, ix, p, *args, levels=levels, return_levels=True),
                                  lambda t, p, m: api.refine_pyramid(t, p, *args, levels=levels, return_levels=True), 3, axis=(0, 1, 1))
    assert lres.shape == (2, 5) and (lsizes > 0).all() and (lsizes[0] < lsizes[1]).all()


def test_score_poses(kit):
    args = (W, H, kit["proj"], kit["sd"], 10)
    (sc,) = _per_mesh(kit, lambda ms, ix, p: (api.score_poses_multi(ms, ix, p, *args),), lambda t, p, m: (api.score_poses(t, p, *args),), 1)
    assert (sc["inlier"] > 0).all() and len(set(sc["inlier"].tolist())) >= 3


def test_score_contours(kit):
    ed = api.scene_edge_distance(kit["sd"], W, H, 10, 3)
    args = (W, H, kit["proj"], kit["sd"], 10, 10, ed)
    sc, con = _per_mesh(kit, lambda ms, ix, p: api.score_contours_multi(ms, ix, p, *args), lambda t, p, m: api.score_contours(t, p, *args), 2)
    assert (con["contour"] > 0).all()


def test_score_normals(kit):
    args = (W, H, kit["proj"], kit["sd"], 10, K, 1, 20, 0.5)
    sc, nrm = _per_mesh(kit, lambda ms, ix, p: api.score_normals_multi(ms, ix, p, *args), lambda t, p, m: api.score_normals(t, p, *args), 2)
    assert nrm["tested"].any() and len(set(nrm["tested"].tolist())) >= 3


def test_pose_information(kit):
    args = (W, H, kit["proj"], K, kit["icp"])
    info, eig, sizes = _per_mesh(kit, lambda ms, ix, p: api.pose_information_multi(ms, ix, p, *args, centers=kit["centers"], radii=kit["radii"]),
                                 lambda t, p, m: api.pose_information(t, p, *args, center=kit["centers"][m], radius=float(kit["radii"][m])), 3)
    assert (sizes > 0).all() and (info["rho"] == kit["radii"][IDX]).all()


def test_contour_information(kit):
    nd = api.scene_edge_nearest(kit["sd"], W, H, 10, 3)
    args = (W, H, kit["proj"], K, kit["sd"], 10, 10, nd)
    sc, fit, info = _per_mesh(kit, lambda ms, ix, p: api.contour_information_multi(ms, ix, p, *args, centers=kit["centers"], radii=kit["radii"]),
                              lambda t, p, m: api.contour_information(t, p, *args, center=kit["centers"][m], radius=float(kit["radii"][m])), 3)
    assert (fit["contour"] > 0).all() and (info["rho"] == kit["radii"][IDX]).all()


def test_pose_vsd_pairs(kit):
    gt = kit["poses"].copy()
    gt[:, 0, 3] += np.array([2.0, -3.0, 4.0, -5.0, 6.0], np.float32)
    args = (W, H, kit["proj"], kit["sd"], K, 15.0, (5.0, 10.0, 20.0))
    got = api.pose_vsd_multi(kit["meshes"], IDX, kit["poses"], gt, *args)
    for m in (0, 2):
        sel = np.flatnonzero(IDX == m)
        assert _same(got[sel], api.pose_vsd(kit["meshes"][m], kit["poses"][sel], gt[sel], *args)), m
    assert (got["uni"] > 0).all() and len(set(got["uni"].tolist())) > 1


# ---- permutation equivariance ------------------------------------------------------------------------------------------------------------
def test_overlap_matrix_permutes_rows_and_columns(kit):
    args = (W, H, kit["proj"], kit["sd"], TAU_ALL)
    sc, ov = api.score_overlap_multi(kit["meshes"], IDX, kit["poses"], *args)
    sc_p, ov_p = api.score_overlap_multi(kit["meshes"], IDX[PI], kit["poses"][PI], *args)
    assert _same(sc_p, sc[PI]) and _same(ov_p, np.ascontiguousarray(ov[np.ix_(PI, PI)]))
    assert (ov[~np.eye(5, dtype=bool)] > 0).all() and not np.array_equal(ov_p, ov)      # every pair shares pixels, also across meshes
    assert np.array_equal(np.diag(ov), sc["inlier"]) and np.array_equal(ov, ov.T)


def test_penetration_permutes_rows_and_columns(kit):
    args = (W, H, kit["proj"], 0)
    pairs = api.pose_penetration_multi(kit["meshes"], IDX, kit["poses"], *args)
    pairs_p = api.pose_penetration_multi(kit["meshes"], IDX[PI], kit["poses"][PI], *args)
    assert _same(pairs_p, np.ascontiguousarray(pairs[np.ix_(PI, PI)]))
    assert (pairs["both"] > 0).all() and len(set(np.diag(pairs["sum_mm"]).tolist())) == 5 and pairs_p.tobytes() != pairs.tobytes()


def test_cover_walk_maps_through_the_permutation(kit):
    args = (W, H, kit["proj"], kit["sd"], TAU_ALL)
    order = np.array([4, 1, 0, 3, 2])
    where = np.argsort(PI)                                         # original index -> index in the permuted call
    sc, cov, frame, sel = api.score_cover_multi(kit["meshes"], IDX, kit["poses"], *args, order, min_new_fraction=(1, 4))
    sc_p, cov_p, frame_p, sel_p = api.score_cover_multi(kit["meshes"], IDX[PI], kit["poses"][PI], *args, where[order], min_new_fraction=(1, 4))
    assert _same(sc_p, sc[PI]) and _same(cov_p, cov[PI]) and frame_p.tobytes() == frame.tobytes()
    assert np.array_equal(PI[sel_p], sel) and 1 < len(sel) <= 5 and sel[0] == order[0]


def test_render_images_follow_the_poses(kit):
    img = api.render_multi(kit["meshes"], IDX, kit["poses"], W, H, kit["proj"]).to_host().reshape(5, H, W)
    img_p = api.render_multi(kit["meshes"], IDX[PI], kit["poses"][PI], W, H, kit["proj"]).to_host().reshape(5, H, W)
    assert np.array_equal(img_p, img[PI]) and all((img[i] > 0).any() for i in range(5))
    for i in range(5):
        assert np.array_equal(img[i], api.render_host(kit["meshes"][IDX[i]], kit["poses"][i:i + 1], W, H, kit["proj"])[0]), i


def test_compose_records_permute(kit):
    """The per-hypothesis records only: the labels carry the caller's index (test_compose_gpu.py holds them)."""
    args = (W, H, kit["proj"], kit["sd"], TAU_ALL)
    _, _, sc, vis, frame = api.compose_detections_multi(kit["meshes"], IDX, kit["poses"], *args)
    _, _, sc_p, vis_p, frame_p = api.compose_detections_multi(kit["meshes"], IDX[PI], kit["poses"][PI], *args)
    assert _same(sc_p, sc[PI]) and _same(vis_p, vis[PI]) and frame_p.tobytes() == frame.tobytes()
    assert (vis["owned"] > 0).all() and len(set(vis["owned"].tolist())) > 1      # every hypothesis keeps pixels, the nearer ones in front
