"""GPU tests (-m gpu): the kernels against float64 geometry (tests/truth_ref.py), directly -- not through the oracle, so each stands even if the oracle is wrong.
Render (render_host, render, render_multi, the fused path's view), depth2cloud, the row convention between the two, device scene preparation and the
projective lookup point by point; and (second half) the refinement loop.  Each assertion is the one tests/test_truth_host.py applies to the oracle, with the same bound (tests/truth_cases.py,
measured on the oracle: profiles/truth/README.md).  Small shapes only: frames of 64 x 48 to 130 x 77, at most 200 triangles and 5 poses per case."""
import numpy as np
import pytest

import oracle_lib as O
import truth_cases as TC
import truth_ref as T
from pose_refine_amd import _lib, api
from test_pass_sums_gpu import icp_batch, options, ragged

pytestmark = pytest.mark.gpu


# ---- render ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,W,H", TC.RENDER_FRAMES)
def test_render_is_the_ray_cast(gpu, seed, W, H):
    """render_host and render (+ to_host), full frame and the two windows, view by view (each view its own mesh: the triangles in front of the camera)."""
    s = TC.render_scene(seed, W, H)
    proj = api.compute_proj(s["K"], W, H)
    for i, v in enumerate(s["views"]):
        model = api.Model(tris=v["tris"])
        pose = v["pose"][None]
        TC.check_render(api.render_host(model, pose, W, H, proj)[0], v["z"], v["edge"], f"render_host seed {seed} view {i}")
        TC.check_render(api.render(model, pose, W, H, proj).to_host().reshape(H, W), v["z"], v["edge"], f"render seed {seed} view {i}")
        for roi in s["rois"]:
            z, edge = TC.window(v["z"], roi), TC.window(v["edge"], roi)
            TC.check_render(api.render_host(model, pose, W, H, proj, roi)[0], z, edge, f"render_host seed {seed} view {i} roi {roi}", cap=False)
            TC.check_render(api.render(model, pose, W, H, proj, roi).to_host().reshape(roi[3], roi[2]), z, edge, f"render seed {seed} view {i} roi {roi}", cap=False)


def test_render_multi_mixed_batch_is_the_ray_cast(gpu):
    seed, W, H = TC.RENDER_FRAMES[0]
    s = TC.render_scene(seed, W, H)
    proj = api.compute_proj(s["K"], W, H)
    a, b = s["views"][1], s["views"][4]                                   # two meshes: what is in front of the camera at 150 mm and at 45 mm
    order = [a, b, b, a]
    poses = np.stack([v["pose"] for v in order])
    idx = np.array([0, 1, 1, 0], np.int32)
    got = api.render_multi([a["tris"], b["tris"]], idx, poses, W, H, proj).to_host().reshape(4, H, W)
    for k, v in enumerate(order):
        TC.check_render(got[k], v["z"], v["edge"], f"render_multi image {k}")
    roi = s["rois"][1]
    got = api.render_multi([a["tris"], b["tris"]], idx, poses, W, H, proj, roi).to_host().reshape(4, roi[3], roi[2])
    for k, v in enumerate(order):
        TC.check_render(got[k], TC.window(v["z"], roi), TC.window(v["edge"], roi), f"render_multi image {k} roi", cap=False)


@pytest.mark.parametrize("seed,W,H", TC.RENDER_FRAMES)
def test_fused_path_sees_the_ray_cast(gpu, seed, W, H):
    """refine_batch renders for itself (pixel boxes, no full frame): its cloud sizes are the truth's hit counts, give or take the pixels of the edge
    band: hits_outside_band <= size <= hits_outside_band + band_pixels."""
    s = TC.render_scene(seed, W, H)
    K = s["K"]
    proj = api.compute_proj(K, W, H)
    v0 = s["views"][0]
    scene = api.Scene_projective().init_Scene_projective_cuda(api.render_host(api.Model(tris=v0["tris"]), v0["pose"][None], W, H, proj)[0], K, W, H)
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 1)
    for i, v in enumerate(s["views"]):
        model = api.Model(tris=v["tris"])
        _, sizes = api.refine_batch(model, v["pose"][None], W, H, proj, K, scene, crit)
        lo, hi = TC.fused_size_bounds(v["z"], v["edge"])
        TC.say(f"fused seed {seed} view {i}: {lo} <= {int(sizes[0])} <= {hi}")
        assert lo <= int(sizes[0]) <= hi
        roi = s["rois"][1]
        _, sizes = api.refine_batch(model, v["pose"][None], W, H, proj, K, scene, crit, roi=roi)
        lo, hi = TC.fused_size_bounds(TC.window(v["z"], roi), TC.window(v["edge"], roi))
        assert lo <= int(sizes[0]) <= hi, (i, roi, lo, int(sizes[0]), hi)


# ---- back-projection ------------------------------------------------------------------------------------------------------------------------
def test_depth2cloud_is_the_back_projection(gpu):
    worst = 0.0
    for d, K, stride, tlx, tly in TC.cloud_cases():
        H, W = d.shape
        got = api.depth2cloud(api.DeviceVector.from_host(d.reshape(-1)), W, H, K, stride, tlx, tly, dtype=d.dtype.type).to_host()
        worst = max(worst, TC.check_cloud(got, d, K, stride, tlx, tly, (d.shape, d.dtype, stride, tlx, tly)))
    TC.say(f"depth2cloud device: largest relative deviation {worst:.3e}")


# ---- render, then back-project, on the device: the row convention ---------------------------------------------------------------------------------
def test_cloud_of_a_render_lies_one_row_off_the_mesh(gpu):
    s = TC.sloped_scene()
    W, H, K = s["W"], s["H"], s["K"]
    depth = api.render(api.Model(tris=s["tris"]), s["pose"][None], W, H, api.compute_proj(K, W, H))
    TC.check_row_pin(api.depth2cloud(depth, W, H, K).to_host(), s["cam"], K, W * H, "device sloped", sloped=True)
    r = TC.render_scene(*TC.RENDER_FRAMES[0])
    W, H, K = r["W"], r["H"], r["K"]
    proj = api.compute_proj(K, W, H)
    for i in (1, 2):
        v = r["views"][i]
        model = api.Model(tris=v["tris"])
        TC.check_row_pin(api.depth2cloud(api.render(model, v["pose"][None], W, H, proj), W, H, K).to_host(), v["cam"], K, W * H, f"device random view {i}")
        roi = r["rois"][1]
        cloud = api.depth2cloud(api.render(model, v["pose"][None], W, H, proj, roi), roi[2], roi[3], K, 1, roi[0], roi[1]).to_host()
        TC.check_row_pin(cloud, v["cam"], K, W * H, f"device random view {i} roi")


# ---- device scene preparation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_device_scene_preparation_on_analytic_surfaces(gpu, dtype):
    """init_Scene_projective_device and init_Scene_nn_device on planes and a sphere: scene points, normals (length, side, angle), the zero border and
    the 2000 mm gate against the truth."""
    W, H, K = TC.NORMAL_W, TC.NORMAL_H, TC.NORMAL_K
    for name, d, n_true in TC.normal_cases():
        dev = api.DeviceVector.from_host(d.astype(dtype).reshape(-1))
        ps = api.Scene_projective().init_Scene_projective_device(dev, K, W, H)
        TC.check_normals(ps.normal_buffer.to_host(), d, n_true, f"proj device {name} {dtype.__name__}")
        TC.check_scene_points(ps.pcd_buffer.to_host(), d, K, name)
        ns = api.Scene_nn().init_Scene_nn_device(dev, K, W, H)
        n = ns._n_points
        assert n == int((d > 0).sum())
        pts, nrm, mask = TC.nn_points_to_pixels(ns.pcd_buffer.to_host()[:3 * n], ns.normal_buffer.to_host()[:3 * n], K, W, H)
        assert np.array_equal(mask, d > 0)
        TC.check_scene_points(pts, d, K, f"nn device {name}")
        TC.check_normals(nrm.reshape(-1, 3), d, n_true, f"nn device {name} {dtype.__name__}")


@pytest.mark.parametrize("image", ["uint16", "int32", "int32_wide"])
def test_device_scene_preparation_on_every_gate_subset(gpu, image):
    """Parity, but on an input that reaches all 256 subsets of the eight tap gates (counted in test_truth_host.py): the noise image as uint16, as
    int32, and as int32 with negative values and values above 65535 -- against the oracle bit for bit."""
    W, H, K = TC.NOISE_W, TC.NOISE_H, TC.NORMAL_K
    d = {"uint16": TC.noise_depth().astype(np.uint16), "int32": TC.noise_depth(), "int32_wide": TC.noise_depth_wide()}[image]
    dev = api.DeviceVector.from_host(d.reshape(-1))
    ref = O.ProjScene(d, K)
    ps = api.Scene_projective().init_Scene_projective_device(dev, K, W, H)
    assert ps.normal_buffer.to_host().tobytes() == ref.normal.tobytes()
    assert ps.pcd_buffer.to_host().tobytes() == ref.pcd.tobytes()
    nref = O.NNScene(d, K)
    ns = api.Scene_nn().init_Scene_nn_device(dev, K, W, H)
    n, m = len(nref.pcd), len(nref.nodes)
    assert (ns._n_points, ns._n_nodes) == (n, m)
    assert ns.pcd_buffer.to_host()[:3 * n].tobytes() == nref.pcd.tobytes() and ns.normal_buffer.to_host()[:3 * n].tobytes() == nref.normal.tobytes()
    assert ns.nodes.to_host()[:m].tobytes() == nref.nodes.tobytes()


# ---- projective lookup, point by point --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", list(TC.LOOKUP_WINDOWS))
def test_lookup_takes_the_pixel_the_projection_says(gpu, name, packed):
    """debug_contrib29 on the hard cloud of truth_cases.lookup_cloud: the scene is made from a depth image (so the packed record is allowed), then only
    its normal buffer is overwritten with normal[pixel] = (1, px / 1024, py / 1024) -- sums 15 .. 17 of a point then name the pixel it took, sum 28 says
    whether it matched.  Outside the boundary band: truth_ref.project's pixel and decision; inside: the oracle's, on one-point clouds.
    The z = 1e-39 block is where proj_pixel's short division used to reject points the reference accepts (a denormal z has no hardware reciprocal:
    all 60 of them, profiles/truth/README.md)."""
    x0, y0, w, h = TC.LOOKUP_WINDOWS[name]
    scene = api.Scene_projective().init_Scene_projective_cuda(TC.lookup_depth(), TC.LOOKUP_K, TC.LOOKUP_W, TC.LOOKUP_H, TC.LOOKUP_MAX_DIST)
    if name != "whole":
        scene = scene.crop((x0, y0, w, h))
    code = TC.pixel_code(w, h)
    api.check(_lib.load().pr_memcpy_h2d(scene.normal_buffer.data(), code.ctypes.data, code.nbytes))
    pts, _ = TC.lookup_cloud(name)
    rows = api.debug_contrib29(api.DeviceVector.from_host(pts.reshape(-1)), scene, packed=packed)
    TC.check_lookup(rows, name, f"device packed={packed}", TC.oracle_lookup_rows(name))


# =================================================================================================================================================
#  The refinement loop on the device against the float64 definitions of tests/truth_ref.py: per-point terms, the pending update, the 29 sums of
#  the product pass, the loop and its fixed point, the fused path.  Assertions and bounds are those of test_truth_host.py (tests/truth_cases.py);
#  the oracle appears only where that file lets it: one-point clouds inside the association band.  The truth is computed from the scene arrays
#  the DEVICE holds.  Frames of 96 x 72, clouds of 936 .. 5436 points; the float64 loops are computed once per module and shared read-only.
# =================================================================================================================================================
A_W, A_H, A_K, A_MAX = TC.ICP_W, TC.ICP_H, TC.ICP_K, TC.ICP_MAX_DIST


def device_scenes(depth):
    """The projective scene from a host depth image (so that the packed record is allowed) and the kd-tree scene built on the device."""
    d = np.array(depth, np.int32)
    proj = api.Scene_projective().init_Scene_projective_cuda(d, A_K, A_W, A_H, A_MAX)
    nn = api.Scene_nn().init_Scene_nn_device(api.DeviceVector.from_host(d.reshape(-1)), A_K, A_W, A_H, max_dist_diff=A_MAX)
    return proj, nn


def scene_truth(scene, kind, name="whole"):
    """(float64 association, scene points, scene normals) from the arrays the device holds."""
    n = scene._n_points if kind == "nn" else scene.width * scene.height
    pcd = scene.pcd_buffer.to_host()[:3 * n].reshape(-1, 3)
    nrm = scene.normal_buffer.to_host()[:3 * n].reshape(-1, 3)
    return (TC.nn_associate(pcd) if kind == "nn" else TC.proj_associate(pcd, TC.ICP_WINDOWS[name])), pcd, nrm


@pytest.fixture(scope="module")
def scenes_a(gpu):
    proj, nn = device_scenes(TC.scene_a_depth())
    out = {("proj", "whole"): proj, ("proj", "cropped"): proj.crop(TC.ICP_WINDOWS["cropped"]), ("nn", "whole"): nn}
    return {k: (s,) + scene_truth(s, *k) for k, s in out.items()}


@pytest.fixture(scope="module")
def loop_truth(scenes_a):
    main, _ = TC.cloud_a_main()
    out = {}
    for kind in ("proj", "nn"):
        _, assoc, pcd, nrm = scenes_a[kind, "whole"]
        out[kind] = T.icp(main, assoc, pcd, nrm, max(TC.LOOP_ITERATIONS))
    return out


# ---- (a) terms, point by point ------------------------------------------------------------------------------------------------------------------
TERM_CASES = [("proj", "whole", False), ("proj", "whole", True), ("proj", "cropped", False), ("proj", "cropped", True), ("nn", "whole", False)]


@pytest.mark.parametrize("kind,name,packed", TERM_CASES)
def test_terms_are_point_to_plane(scenes_a, kind, name, packed):
    """debug_contrib29 on cloud A with all its blocks: arrays and packed record, whole and cropped; the kd-tree scene built by init_Scene_nn_device."""
    cloud, block, _ = TC.cloud_a()
    scene, assoc, pcd, nrm = scenes_a[kind, name]
    rows = api.debug_contrib29(api.DeviceVector.from_host(cloud.reshape(-1)), scene, packed=packed)
    truth = TC.truth_terms((kind, name, "a"), cloud, assoc, pcd, nrm)
    TC.check_terms(rows, cloud, block, truth, f"device {kind} {name} packed={packed}", TC.oracle_rows_of(TC.scene_a_oracle(kind, name)))


# ---- (b) the pending update ------------------------------------------------------------------------------------------------------------------------
def updates(scenes_a):
    main, _ = TC.cloud_a_main()
    _, assoc, pcd, nrm = scenes_a["proj", "whole"]
    return TC.given_updates(T.float64_truth(TC.truth_terms(("proj", "main"), main, assoc, pcd, nrm)[0].sum(0))[0])


@pytest.mark.parametrize("which", ["pass0", "20deg"])
@pytest.mark.parametrize("kind,name,packed", [("proj", "whole", False), ("proj", "whole", True), ("nn", "whole", False)])
def test_pending_update_moves_the_cloud_and_the_terms_follow(scenes_a, kind, name, packed, which):
    """debug_contrib29(update=M): the cloud the kernel wrote back is R p + t, and the terms are the float64 terms OF THE FLOAT32 CLOUD IT WROTE BACK
    (so that the update's rounding is not counted a second time)."""
    main, _ = TC.cloud_a_main()
    M = updates(scenes_a)[which]
    scene, assoc, pcd, nrm = scenes_a[kind, name]
    dev = api.DeviceVector.from_host(main.reshape(-1))
    rows = api.debug_contrib29(dev, scene, update=M, packed=packed)
    moved = dev.to_host().reshape(-1, 3)
    TC.check_moved(moved, M, main, f"device {kind} packed={packed} {which}", TC.MOVED_GIVEN_UNITS_MEASURED)
    truth = TC.truth_terms((kind, name, which), moved, assoc, pcd, nrm)
    TC.check_terms(rows, moved, np.full(len(moved), "main"), truth, f"device {kind} packed={packed} after {which}", TC.oracle_rows_of(TC.scene_a_oracle(kind, name)), min_accept=300)


# ---- (c) the 29 sums of the product pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppb", TC.SUM_PPBS)
@pytest.mark.parametrize("kind,cfg", [("proj", {}), ("nn", {}), ("nn", dict(nn_split=1))], ids=["proj", "nn-default", "nn-split"])
def test_pass_sums_are_the_sums_of_the_terms(scenes_a, kind, cfg, ppb):
    """One ragged ICP_Point2Plane_batch of the windows of cloud A under api.trace_sums, criteria (0, 0, 1): row 0 of every window against the float64
    sum of its float64 terms."""
    main, _ = TC.cloud_a_main()
    scene, assoc, pcd, nrm = scenes_a[kind, "whole"]
    t64, sc, _, _ = TC.truth_terms((kind, "main"), main, assoc, pcd, nrm)
    sizes = TC.SUM_SIZES + (len(main),)
    flat, offs = ragged([main[:n] for n in sizes])
    with options(points_per_block=ppb, **cfg):
        rows = api.trace_sums(len(sizes), 2)
        icp_batch(flat, offs, scene, (0.0, 0.0, 1))
    assert not np.isnan(rows[0]).any()
    worst = {n: TC.check_sums(rows[0, i], t64[:n], sc[:n], ppb, f"device {kind} {cfg} {n} points") for i, n in enumerate(sizes)}
    TC.say(f"sums device {kind} {cfg} ppb {ppb}: units of 2^-24 of the summed scales per window {({k: round(v, 3) for k, v in worst.items()})}; max {max(worst.values()):.3f}")


# ---- (d) the loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", ["host", "device"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_loop_follows_the_float64_loop_to_the_known_motion(scenes_a, loop_truth, kind, solve):
    main, M = TC.cloud_a_main()
    known = np.linalg.inv(M)
    scene = scenes_a[kind, "whole"][0]
    offs = np.array([0, len(main)], np.uint32)
    with options(points_per_block=TC.ICP_PPB, solve=api.SOLVE_DEVICE if solve == "device" else api.SOLVE_HOST):
        for N in TC.LOOP_ITERATIONS:
            rec = icp_batch(main, offs, scene, (0.0, 0.0, N))[0]
            TC.check_loop(rec["T"], rec["fitness"], rec["inlier_rmse"], loop_truth[kind], N, main, known, f"device {kind} {solve} solve")


# ---- (e) the fused path --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_b(gpu):
    """Scene B on the device, the clouds the device renders of the eight hypotheses and the float64 loop started from each, per scene kind."""
    sb = TC.scene_b()
    proj = api.compute_proj(A_K, A_W, A_H)
    model = api.Model(tris=sb["tris"])
    clouds = [api.depth2cloud(api.render(model, sb["hyps"][i:i + 1], A_W, A_H, proj), A_W, A_H, A_K).to_host().reshape(-1, 3) for i in range(len(sb["hyps"]))]
    out = dict(model=model, projection=proj, clouds=clouds)
    for kind, scene in zip(("proj", "nn"), device_scenes(sb["depth"])):
        assoc, pcd, nrm = scene_truth(scene, kind)
        out[kind] = dict(scene=scene, assoc=assoc, pcd=pcd, nrm=nrm, truths=[T.icp(cl, assoc, pcd, nrm, TC.FUSED_ITERATIONS) for cl in clouds])
    return out


@pytest.mark.parametrize("solve", ["host", "device"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_fused_path_follows_the_float64_loop(fused_b, kind, solve):
    """api.refine_batch on scene B, eight hypotheses: the comparison of test_truth_host.py's fused test, started from api.depth2cloud(api.render(...));
    every compared hypothesis ends nearer to the true pose than it started (ADD over the mesh vertices).  Under host solve the sums of every
    hypothesis' first pass are held to the float64 sums of its cloud as well."""
    sb, f = TC.scene_b(), fused_b[kind]
    crit = api.ICPConvergenceCriteria(0.0, 0.0, TC.FUSED_ITERATIONS)
    with options(points_per_block=TC.ICP_PPB, solve=api.SOLVE_DEVICE if solve == "device" else api.SOLVE_HOST):
        rows = api.trace_sums(len(sb["hyps"]), TC.FUSED_ITERATIONS + 1) if solve == "host" else None
        res, sizes = api.refine_batch(fused_b["model"], sb["hyps"], A_W, A_H, fused_b["projection"], A_K, f["scene"], crit)
    assert np.array_equal(sizes, [len(c) for c in fused_b["clouds"]])
    TC.check_fused(res, fused_b["clouds"], f["truths"], kind, f"device {kind} {solve} solve")
    if rows is not None:
        TC.check_fused_sums(rows[0], fused_b["clouds"], f["assoc"], f["pcd"], f["nrm"], ("fused", kind), f"device {kind}")
