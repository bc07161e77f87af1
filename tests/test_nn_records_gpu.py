"""GPU tests (-m gpu): the traversal data the library derives from a kd-tree scene (api.debug_nn_records: topology and boxes, 64-, 32- and
128-byte records, the padded points, the pixel grid) held to the tree and the points it encodes by nn_records_ref.check_records --
on one-leaf trees, lattices full of ties, leaves at and past the wide records' limit, a level of wide nodes that crosses the numbering
kernel's chunk seam, a tree deep enough for the second round of wide levels, scenes on both sides of the frame tests, and grids with
and without a cell per point."""
import ctypes as C

import numpy as np
import pytest

import nn_records_ref as N
import nn_ref
import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import TOL_T, make_scene

pytestmark = pytest.mark.gpu

FIELDS = ("topo", "bmin", "bmax", "rec64", "rec32", "desc", "pts", "info", "wide", "cell_idx", "grid")


def records(scene, camera=None):
    R = api.debug_nn_records(scene, camera)
    R["grid_usable"] = R["counts"]["grid_usable"]
    return R


def same_bytes(a, b, skip_info=()):
    for f in FIELDS:
        x, y = a[f], b[f]
        assert (x is None) == (y is None), f
        if x is None:
            continue
        if f == "info" and skip_info:
            x, y = np.delete(x, skip_info), np.delete(y, skip_info)
        assert x.tobytes() == y.tobytes(), f
    assert a["counts"] == b["counts"]


def host_arrays(scene):
    """The caller's nodes and points of a scene, whichever side built them."""
    if scene.nodes_host is not None:
        return scene.nodes_host, scene.pcd_host
    return (np.ascontiguousarray(scene.nodes.to_host()[:scene._n_nodes]),
            np.ascontiguousarray(scene.pcd_buffer.to_host().reshape(-1, 3)[:scene._n_points]))


def check(scene, camera=None, n_queries=48, frame_rule=True):
    nodes, pts = host_arrays(scene)
    R = records(scene, camera)
    rep = N.check_records(nodes, pts, scene.max_dist_diff, R, camera, n_queries=n_queries)
    if frame_rule and nodes["child1"][0] >= 0:                       # (a one-leaf tree's frame is its points' hull; its bbox is not filled in)
        assert int(R["info"][20]) == int(nn_ref.wide_frame_ok(nodes, scene.max_dist_diff))
    print("nn_records", rep)
    return R, rep


def normals(n, seed=1):
    nrm = np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)
    return np.ascontiguousarray((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32))


def point_scene(pts, max_leaf, max_dist=0.1):
    pts = np.array(pts, np.float32, order="C", copy=True)
    return make_scene(pts, normals(len(pts)), max_leaf, max_dist)


@pytest.fixture(scope="module")
def small_depth():
    f = nn_ref.f3_small(97, 61)
    cam = (f.W, f.H, float(f.K[0]), float(f.K[4]), float(f.K[2]), float(f.K[5]))
    return f, cam


@pytest.mark.parametrize("n", [1, 2, 11])
def test_one_leaf_trees(gpu, n):
    s = point_scene(N.random_points(n, 10 + n), 15)
    assert len(s.nodes_host) == 1
    R, rep = check(s)
    assert rep["wide_usable"] == 1 and rep["n_wide"] == 1 and R["info"][0] == 0


@pytest.mark.parametrize("max_leaf", [1, 3])
def test_lattice_of_ties_and_zero_extent_boxes(gpu, max_leaf):
    _, rep = check(point_scene(N.lattice_points(700, 0.1), max_leaf))
    assert rep["wide_usable"] == 1


def test_random_points(gpu):
    _, rep = check(point_scene(N.random_points(5000, 2), 10, 0.02))
    assert rep["wide_usable"] == 1 and rep["wide_levels"] >= 4


@pytest.mark.parametrize("max_leaf,wide", [(15, 1), (16, 0)])
def test_leaves_at_and_past_the_leaf_reference_limit(gpu, max_leaf, wide):
    s = point_scene(N.random_points(3000, 3), max_leaf, 0.02)
    cnt = (s.nodes_host["right"] - s.nodes_host["left"])[s.nodes_host["child1"] < 0]
    assert cnt.max() == max_leaf
    R, rep = check(s)
    assert rep["wide_usable"] == wide == int(R["info"][8]) and R["info"][1] == 1


def test_level_of_wide_nodes_across_the_chunk_seam(gpu):
    _, rep = check(point_scene(N.random_points(40000, 4), 1, 0.02), n_queries=8)
    assert any(s > N.K_WIDE_CHUNK and s % N.K_WIDE_CHUNK for s in rep["level_sizes"]), rep["level_sizes"]


def test_depth_scene_with_its_grid(gpu, small_depth):
    f, cam = small_depth
    s = api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(f.depth.reshape(-1)), f.K, f.W, f.H)
    R, rep = check(s, cam)
    assert rep["grid_usable"] and R["counts"]["grid_cells"] == N.grid_cells(f.W, f.H) and (R["cell_idx"] >= 0).sum() == s._n_points
    assert records(s)["grid"] is None and records(s)["counts"]["grid_w"] == 0      # no camera: no grid reported


@pytest.mark.parametrize("how", ["two_in_one_cell", "outside_the_image"])
def test_depth_scene_whose_grid_is_not_usable(gpu, small_depth, how):
    f, cam = small_depth
    pts = O.depth2cloud(f.depth, f.K).copy()
    px, py, ok = N.grid_pixels(pts, cam)
    assert ok.all() and len(np.unique(py * f.W + px)) == len(pts)
    if how == "two_in_one_cell":
        cell = set((py * f.W + px).tolist())
        i = next(k for k in range(len(pts) // 2, len(pts)) if int(py[k] * f.W + px[k] + 1) in cell and px[k] + 1 < f.W)
        j = int(np.flatnonzero((py == py[i]) & (px == px[i] + 1))[0])             # the neighbour to the right
        pts[i] = pts[j] * np.float32(1.00001)
    else:
        pts[len(pts) // 3, 0] = np.float32(-2.0 * pts[len(pts) // 3, 2])
    assert not N.build_grid(pts, cam)[0]
    R, rep = check(point_scene(pts, 10), cam)
    assert R["grid"] is not None and not rep["grid_usable"] and R["counts"]["grid_usable"] == 0


@pytest.mark.parametrize("kind", nn_ref.DEGENERATE)
def test_degenerate_point_sets_and_both_sides_of_the_frame_test(gpu, kind):
    f = nn_ref.degenerate(kind)
    R, rep = check(make_scene(f.pts.copy(), f.nrm.copy(), f.max_leaf, f.max_dist))
    assert int(R["info"][20]) == (0 if kind == "far60" else 1) == rep["wide_usable"]


def comb_scene():
    nodes, pts, nrm = N.comb_tree()
    s = api.Scene_nn()
    s.max_dist_diff = 0.003
    s.pcd_host, s.normal_host, s.nodes_host = pts, nrm, nodes
    s.pcd_buffer, s.normal_buffer, s.nodes = api.DeviceVector.from_host(pts.reshape(-1)), api.DeviceVector.from_host(nrm.reshape(-1)), api.DeviceVector.from_host(nodes)
    return s


@pytest.mark.device_solve
def test_comb_tree_takes_the_second_round_of_wide_levels(gpu):
    s = comb_scene()
    R, rep = check(s)
    assert rep["continued"] and rep["wide_levels"] > 16 and 16 < rep["depth"] <= 24 and R["info"][8] == 1
    # a cloud a degree and 3 mm off the scene's own points, 1 mm of noise: most queries end deep in the spine, some beyond the radius
    rng = np.random.default_rng(8)
    base = s.pcd_host[rng.integers(0, len(s.pcd_host), 1500)] + rng.normal(size=(1500, 3)).astype(np.float32) * np.float32(0.001)
    cloud = nn_ref.rigid(base.astype(np.float32), 1.0, 0.003, rng)
    osc = O.NNScene.from_points(s.pcd_host, s.normal_host, s.max_dist_diff, nodes=s.nodes_host)
    ref, _, _, _ = O.icp(cloud, osc, (0.0, 0.0, 2), O.SUM_CANONICAL, api.get_option("points_per_block"))
    got = api.ICP_Point2Plane(api.DeviceVector.from_host(cloud.reshape(-1)), s, api.ICPConvergenceCriteria(0.0, 0.0, 2))
    assert 0.5 < float(ref["fitness"]) < 1.0
    assert got.fitness_ == float(ref["fitness"]) and np.allclose(got.transformation_.reshape(-1), ref["T"], rtol=0, atol=TOL_T)


def test_odd_and_malformed_trees(gpu, small_depth):
    f, cam = small_depth
    s = api.Scene_nn().init_Scene_nn_cuda(f.depth, f.K)
    good = records(s, cam)
    nodes = s.nodes_host.copy()
    # a legal tree whose split values are not between the children: the exact 64-byte records only
    odd = nodes.copy()
    internal = np.flatnonzero(odd["child1"] >= 0)
    odd["split_v"][internal[::3]] += np.float32(0.02)
    s.nodes_host, s.nodes = odd, api.DeviceVector.from_host(odd)
    R, rep = check(s)
    assert R["info"][1] == 0 and R["info"][8] == 0
    # links that do not form a tree: the searches' error, and nothing written
    lib = _lib.load()
    for which in ("child_outside", "parent_disagrees"):
        bad = nodes.copy()
        if which == "child_outside":
            bad["child2"][0] = len(bad) + 5
        else:
            bad["parent"][bad["child1"][0]] = 3
        s.nodes_host, s.nodes = bad, api.DeviceVector.from_host(bad)
        arrs = {k: np.empty_like(good[k]) for k in FIELDS}
        for a in arrs.values():
            a.view(np.uint8)[...] = 0x5A
        cnt = _lib.NNRecordsCounts(*([0x5A5A5A5A] * 7))
        out = _lib.NNRecordsOut(*[arrs[k].ctypes.data for k in FIELDS])
        d = s.desc()
        k4 = np.array(cam[2:], np.float32)
        assert lib.pr_debug_nn_records(C.addressof(d), cam[0], cam[1], k4.ctypes.data, C.byref(cnt), C.byref(out)) == _lib.PR_ERR_INVALID
        assert b"do not form a consistent tree" in lib.pr_last_error()
        assert all((arrs[k].view(np.uint8) == 0x5A).all() for k in FIELDS) and cnt.n_nodes == 0x5A5A5A5A and cnt.grid_cells == 0x5A5A5A5A
    s.nodes_host, s.nodes = nodes, api.DeviceVector.from_host(nodes)
    same_bytes(records(s, cam), good)


def test_builds_are_deterministic(gpu, small_depth):
    f, cam = small_depth
    host = api.Scene_nn().init_Scene_nn_cuda(f.depth, f.K)
    dev = api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(f.depth.reshape(-1)), f.K, f.W, f.H)
    big = point_scene(N.random_points(40000, 4), 1, 0.02)
    api.set_option("scene_cache", 0)
    try:
        same_bytes(records(big), records(big))
        a = records(host, cam)
        same_bytes(a, records(host, cam))
        same_bytes(a, records(dev, cam), skip_info=(12, 13, 14, 15))             # (the cache's fingerprint words cover the normals too)
    finally:
        api.set_option("scene_cache", 1)


@pytest.mark.device_solve
def test_reads_leave_the_cache_and_a_batch_in_flight_alone(gpu, model, scenario, gscenes):
    s = gscenes["nn"]
    K, W, H = scenario["K"], synth.WIDTH, synth.HEIGHT
    cam = (W, H, float(K[0]), float(K[4]), float(K[2]), float(K[5]))
    before = records(s, cam)
    assert before["counts"]["grid_usable"] == 1 and before["info"][8] == 1
    cloud = scenario["cloud"][:4096]
    api.ICP_Point2Plane(api.DeviceVector.from_host(cloud.reshape(-1)), s, api.ICPConvergenceCriteria(0.0, 0.0, 2))
    same_bytes(records(s, cam), before)
    poses, crit = synth.hypotheses(8), api.ICPConvergenceCriteria(0.0, 0.0, 3)
    want, want_sizes = api.refine_batch(model, poses, W, H, scenario["proj"], K, s, crit)
    api.refine_submit(0, model, poses, W, H, scenario["proj"], K, s, crit)
    during = records(s, cam)
    got, sizes = api.refine_wait(0)
    same_bytes(during, before)
    assert got.tobytes() == want.tobytes() and np.array_equal(sizes, want_sizes)
    same_bytes(records(s, cam), before)
