"""Scenes from point clouds on the device: pr_cloud_knn_dev / pr_cloud_normals_dev / pr_scene_nn_from_cloud_dev / pr_ppf_cloud_points_dev against the
host twins (which test_cloud_host.py holds to the numpy restatement), byte for byte, on the smallest clouds that can go wrong; then a scene made
from the points of the scenario's frame next to the depth-built scene of the same frame.  Every check prints its figures before it asserts."""
import functools
import math

import numpy as np
import pytest

import cloud_ref as R
from gpu_common import make_scene
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [c["name"] for c in CASES]


def say(*a):
    print("[cloud]", *a)


def case(name):
    return next(c for c in CASES if c["name"] == name)


def device_scene(c):
    """The case's cloud as a device scene over the HOST-built tree (the twins walk the very same nodes), normals zero."""
    pts = np.array(c["points"], np.float32, order="C")
    return make_scene(pts, np.zeros_like(pts), c["max_leaf"])


def scene_normals(scene):
    return scene.normal_buffer.to_host().reshape(-1, 3)


@pytest.mark.parametrize("name", IDS)
def test_device_equals_twins(gpu, name):
    """idx, d2, count, normals, variation and counts of the kernels equal the host twins' byte for byte."""
    c = case(name)
    scene = device_scene(c)
    p = api.CloudParams(k=c["k"], max_radius=c["max_radius"])
    idx, d2, cnt = api.cloud_knn(scene, p)
    hidx, hd2, hcnt = api.cloud_knn_host(scene.pcd_host, scene.nodes_host, p)
    nrm, var, counts = api.cloud_normals(scene, p, want_variation=True)
    hnrm, hvar, hcounts = api.cloud_normals_host(scene.pcd_host, scene.nodes_host, p)
    say(name, counts)
    assert idx.tobytes() == hidx.tobytes() and d2.tobytes() == hd2.tobytes() and cnt.tobytes() == hcnt.tobytes()
    assert counts == hcounts
    assert nrm.to_host().tobytes() == hnrm.tobytes() and var.to_host().tobytes() == hvar.tobytes()


def test_in_place_and_twice(gpu):
    """Normals written into the scene's own array equal those written elsewhere; a second call gives the same bytes; an ICP call on the scene
    afterwards reads the new normals (no stale derived form)."""
    c = case("n257")
    scene = device_scene(c)
    p = api.CloudParams(k=c["k"])
    want, _, _ = api.cloud_normals_host(scene.pcd_host, scene.nodes_host, p)
    api.cloud_knn(scene, p)                                              # the scene's derived records exist from here on
    out, _, counts = api.cloud_normals(scene, p, in_place=True)
    assert out is scene.normal_buffer and scene_normals(scene).tobytes() == want.tobytes()
    api.cloud_normals(scene, p, in_place=True)
    assert scene_normals(scene).tobytes() == want.tobytes()
    idx1 = api.cloud_knn(scene, p)
    idx2 = api.cloud_knn(scene, p)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(idx1, idx2))
    # the same ICP call against a fresh scene that was made with these normals
    fresh = make_scene(scene.pcd_host.copy(), want.copy(), c["max_leaf"])
    cloud2 = api.DeviceVector.from_host(scene.pcd_host[:64].reshape(-1) + np.float32(0.001))
    cloud3 = api.DeviceVector.from_host(scene.pcd_host[:64].reshape(-1) + np.float32(0.001))
    a = api.ICP_Point2Plane(cloud2, scene, api.ICPConvergenceCriteria(0.0, 0.0, 1))
    b = api.ICP_Point2Plane(cloud3, fresh, api.ICPConvergenceCriteria(0.0, 0.0, 1))
    say("ICP after the in-place write: fitness", a.fitness_, "rmse", a.inlier_rmse_)
    assert a.fitness_ > 0 and a.transformation_.tobytes() == b.transformation_.tobytes() and a.inlier_rmse_ == b.inlier_rmse_ and a.fitness_ == b.fitness_


@pytest.mark.parametrize("name", ["n65", "random2000_leaf10_k16_rinf", "lattice"])
def test_scene_from_cloud(gpu, name):
    """init_Scene_nn_cloud: the device build of the tree equals the host build, the normals the host twin's over it; desc() carries no camera."""
    c = case(name)
    scene = api.Scene_nn().init_Scene_nn_cloud(c["points"], k=c["k"], max_radius=c["max_radius"], max_leaf=c["max_leaf"])
    pts, nodes = api.kdtree_build_host(c["points"], c["max_leaf"])
    d = scene.desc()
    assert (d.n_points, d.n_nodes, d.cam_magic, d.cam_w) == (len(pts), len(nodes), 0, 0) and scene.camera is None
    assert scene.pcd_buffer.to_host().tobytes() == pts.tobytes()
    assert scene.nodes.to_host()[:len(nodes)].tobytes() == nodes.tobytes()
    want, _, counts = api.cloud_normals_host(pts, nodes, k=c["k"], max_radius=c["max_radius"])
    assert scene_normals(scene).tobytes() == want.tobytes() and scene.cloud_counts == counts
    # a DeviceVector is adopted and reordered in place
    dv = api.DeviceVector.from_host(np.ascontiguousarray(c["points"], np.float32).reshape(-1))
    again = api.Scene_nn().init_Scene_nn_cloud(dv, k=c["k"], max_radius=c["max_radius"], max_leaf=c["max_leaf"])
    assert again.pcd_buffer is dv and dv.to_host().tobytes() == pts.tobytes() and scene_normals(again).tobytes() == want.tobytes()


def test_ppf_cloud_points(gpu):
    """The strided sample equals a numpy gather, points without a normal are skipped, and the cap is pr_ppf_scene_points_dev's error."""
    c = case("random2000_leaf10_k8_r0.12")                               # four of its points have too few neighbours: no normal
    scene = api.Scene_nn().init_Scene_nn_cloud(c["points"], k=c["k"], max_radius=c["max_radius"], max_leaf=c["max_leaf"])
    pcd, nrm = scene.pcd_buffer.to_host().reshape(-1, 3), scene_normals(scene)
    none = np.flatnonzero(~(nrm != 0).any(axis=1))
    assert len(none) == scene.cloud_counts["too_few"] == 4
    for stride in (1, 3, 7, 2000, 5000) + tuple(int(s) for s in none[:2] if s > 0):      # the last two: a sample that lands on a point without a normal
        pts_d, nrm_d, n = api.ppf_cloud_points(scene, stride)
        pick = np.arange(0, len(pcd), stride)
        pick = pick[(nrm[pick] != 0).any(axis=1)]
        say("stride", stride, "kept", n, "of", len(np.arange(0, len(pcd), stride)))
        assert n == len(pick)
        assert pts_d.to_host()[:3 * n].tobytes() == (pcd[pick] * np.float32(1000.0)).tobytes()
        assert nrm_d.to_host()[:3 * n].tobytes() == nrm[pick].tobytes()
    with pytest.raises(api.PoseRefineError):
        api.ppf_cloud_points(scene, 0)
    big = api.Scene_nn().init_Scene_nn_cloud(R.random_cloud(api.PPF_MAX_SCENE_POINTS + 300, 77), k=8)
    assert big.cloud_counts["with_normal"] == api.PPF_MAX_SCENE_POINTS + 300
    with pytest.raises(api.PoseRefineError) as e:
        api.ppf_cloud_points(big, 1)
    assert e.value.code == _lib.PR_ERR_INVALID and "PR_PPF_MAX_SCENE_POINTS" in str(e.value)
    _, _, n = api.ppf_cloud_points(big, 2)
    assert n == (api.PPF_MAX_SCENE_POINTS + 300 + 1) // 2


# ---- end to end on the scenario's frame ---------------------------------------------------------------------------------------------------------
def perturbed(pose, n=8, seed=3):
    """n small perturbations of a pose: up to 2 degrees about each axis and 3 mm along each."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 4, 4), np.float32)
    for i in range(n):
        r = synth.euler_zyx(np.radians(rng.uniform(-2.0, 2.0, 3)).astype(np.float32))
        out[i] = synth.pose_matrix((r.astype(np.float64) @ pose[:3, :3].astype(np.float64)).astype(np.float32), (pose[:3, 3] + rng.uniform(-3.0, 3.0, 3)).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def cloud_scene(gpu, gscenes):
    """The points of the depth-built scene of frame 1, handed over as a bare cloud in the order the depth path's builder met them (row-major over
    the frame's valid pixels).  pr_kdtree_build's two-ended partition is not stable, so building from the points in TREE order is no fixed point
    (leaf contents come out permuted, and with the frame's tied coordinates some splits move): only the builder's own input order gives the same
    builder the same input."""
    depth_scene = gscenes["nn"]
    dense = gscenes["proj"].pcd_host.reshape(-1, 3)
    pixel_order = np.ascontiguousarray(dense[dense[:, 2] > 0])
    tree_order = depth_scene.pcd_host
    key = lambda a: a[np.lexsort(a.T[::-1])].tobytes()
    assert len(pixel_order) == len(tree_order) and key(pixel_order) == key(tree_order)       # the same points
    return api.Scene_nn().init_Scene_nn_cloud(pixel_order, max_leaf=10)


def test_scenario_tree_equals_depth_built(gpu, gscenes, cloud_scene):
    depth_scene = gscenes["nn"]
    assert cloud_scene.pcd_buffer.to_host().tobytes() == depth_scene.pcd_host.tobytes()
    assert cloud_scene.nodes.to_host()[:len(depth_scene.nodes_host)].tobytes() == depth_scene.nodes_host.tobytes()
    assert cloud_scene.desc().n_nodes == len(depth_scene.nodes_host)
    a = np.degrees(R.angle(scene_normals(cloud_scene), depth_scene.normal_host, signed=True))
    say("cloud scene", cloud_scene.cloud_counts, "angle to the stencil's normals, degrees: median %.2f, 90 %% %.2f" % (np.median(a), np.percentile(a, 90)))


def test_scenario_refine_against_both_scenes(gpu, model, scenario, gscenes, cloud_scene):
    """Eight small perturbations of the scene pose refined against the depth-built scene, the cloud scene and a Scene_grid of the cloud scene.
    max_displacement (MSSD) to the known pose, the largest of the eight, measured on one MI355X: 0.2238 mm against the depth-built scene, 0.2145 mm against the
    cloud scene (k = 16; its normals lie a median 7.7 degrees off the stencil's), 0.1407 mm against the grid; the cloud scene is held to the larger of twice the depth-built scene's figure and that figure plus 1 mm (the frame's depth quantum)."""
    W, H, K = synth.WIDTH, synth.HEIGHT, scenario["K"]
    gt = synth.scene_pose()
    hyp = perturbed(gt)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
    figures = {}
    grid = api.Scene_grid.from_scene_nn(cloud_scene, 0.004)
    for name, scene in (("depth", gscenes["nn"]), ("cloud", cloud_scene), ("grid of cloud", grid)):
        res, _ = api.refine_batch(model, hyp, W, H, scenario["proj"], K, scene, crit)
        mssd = api.max_displacement(api.pose_distance(model, api.refined_poses(res, hyp), gt))
        figures[name] = float(mssd.max())
        say(name, "MSSD mm per hypothesis", np.round(mssd, 4), "fitness", np.round(res["fitness"], 4))
        assert np.isfinite(mssd).all() and (res["fitness"] > 0).all()
    start = api.max_displacement(api.pose_distance(model, hyp, gt))
    say("before refinement: MSSD mm", np.round(start, 3), "| largest after:", figures)
    assert figures["cloud"] <= max(2.0 * figures["depth"], figures["depth"] + 1.0)


def test_scenario_hypotheses_from_cloud(gpu, model, cloud_scene):
    """generate_hypotheses from the cloud scene's sample alone puts a hypothesis with ADD < 0.1 d into its list."""
    pm = api.PPFModel(model)
    sample = api.ppf_cloud_points(cloud_scene, 16)                       # every 16th point of tree order: the depth route's density at its default stride 4 (every 4th column of every 4th row)
    hyp, votes = api.generate_hypotheses(pm, None, scene_sample=sample)
    assert 0 < len(hyp) <= 256 and np.all(np.diff(votes) <= 0)
    v64 = model.vertices.astype(np.float64)
    sq = (v64 * v64).sum(1)
    diam = math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))
    add = api.mean_displacement(api.pose_distance(model, hyp, synth.scene_pose()))
    good = np.flatnonzero(add < 0.1 * diam)
    say("sample", sample[2], "hypotheses", len(hyp), "with ADD < 0.1 d:", len(good), "first at rank", int(good[0]) + 1 if len(good) else None, "best ADD mm", float(add.min()))
    assert len(good) > 0
    # the same keyword on the multi entry: one model's slice equals the single call
    mi, hm, vm = api.generate_hypotheses_multi([pm], None, scene_sample=sample)
    assert hm.tobytes() == hyp.tobytes() and vm.tobytes() == votes.tobytes() and (mi == 0).all()
