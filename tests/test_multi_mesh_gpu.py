"""GPU tests (-m gpu) of mixed batches (pr_render_multi / pr_refine_batch_multi / pr_score_poses_multi): hypotheses of several meshes in
one call.  Every output is held byte for byte to the single-mesh call for the same mesh and poses, and a 24-pose mixed batch to the oracle."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O
import seam_cases as S
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H, TOL_T, inliers, random_mesh
from verify_ref import launch_split_case

pytestmark = pytest.mark.gpu

CRIT = api.ICPConvergenceCriteria(0.0, 0.0, 10)
ROI = (100, 80, 420, 330)


def _rigid(tris, angle, t):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    return np.ascontiguousarray((tris.reshape(-1, 3) @ R.T + np.asarray(t, np.float32)).astype(np.float32).reshape(-1, 3, 3))


@pytest.fixture(scope="module")
def meshes(gpu, scenario):
    """obj_06, a rigidly re-posed copy, a scaled copy and a random soup -- as Model, DeviceVector and host array."""
    t = scenario["tris"]
    rng = np.random.default_rng(11)
    return [api.Model(tris=t), api.DeviceVector.from_host(_rigid(t, 0.3, (4.0, -3.0, 2.0)).reshape(-1)),
            np.ascontiguousarray(t * np.float32(0.8)), random_mesh(rng, 3000, 25.0)]


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)


def _assignments(P, n):
    return {"interleaved": np.arange(P) % n, "random": np.random.default_rng(7).integers(0, n, P)}


def _refine_single(meshes, idx, poses, scene, roi=None, crit=CRIT):
    """What one refine_batch call per mesh gives, in pose order (the configs[1] camera)."""
    proj, K = O.compute_proj(synth.K_TEST, W, H), synth.K_TEST
    res = np.zeros(len(poses), _lib.RESULT)
    sizes = np.zeros(len(poses), np.uint32)
    for m in range(len(meshes)):
        sel = np.flatnonzero(idx == m)
        if len(sel):
            res[sel], sizes[sel] = api.refine_batch(meshes[m], poses[sel], W, H, proj, K, scene, crit, roi=roi)
    return res, sizes


def _assert_refine_equal(got, want):
    assert np.array_equal(got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes()


# ---- parity with the single-mesh calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assign", ["interleaved", "random"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
@pytest.mark.parametrize("roi", [None, ROI])
def test_refine_parity(gpu, scenario, gscenes, meshes, hyps, assign, kind, solve, roi):
    idx = _assignments(len(hyps), len(meshes))[assign]
    api.set_option("solve", solve)
    try:
        got = api.refine_batch_multi(meshes, idx, hyps, W, H, scenario["proj"], scenario["K"], gscenes[kind], CRIT, roi=roi)
        want = _refine_single(meshes, idx, hyps, gscenes[kind], roi)
    finally:
        api.set_option("solve", api.SOLVE_HOST)
    _assert_refine_equal(got, want)
    assert (got[1] > 0).sum() > len(hyps) // 2                   # most hypotheses see their object


def test_refine_against_oracle(gpu, scenario, gscenes, meshes):
    poses = synth.hypotheses(24)
    idx = np.arange(24) % len(meshes)
    crit = (0.0, 0.0, 20)
    res, sizes = api.refine_batch_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], api.ICPConvergenceCriteria(*crit))
    host = [scenario["tris"], _rigid(scenario["tris"], 0.3, (4.0, -3.0, 2.0)), meshes[2], meshes[3]]
    for m in range(len(meshes)):
        sel = np.flatnonzero(idx == m)
        ores, osizes, _ = O.refine_batch(host[m], poses[sel], W, H, scenario["proj"], scenario["K"], scenario["proj_scene"], crit,
                                         O.SUM_CANONICAL, api.get_option("points_per_block"))
        assert np.array_equal(sizes[sel], osizes), m
        assert np.array_equal(inliers(res["fitness"][sel], sizes[sel]), inliers(ores["fitness"], osizes)), m
        assert np.array_equal(res["fitness"][sel], ores["fitness"]), m
        assert np.allclose(res["inlier_rmse"][sel], ores["inlier_rmse"], rtol=1e-6, atol=0), m
        assert np.allclose(res["T"][sel], ores["T"], rtol=0, atol=TOL_T), m


@pytest.fixture(scope="module")
def noisy(scenario):
    rng = np.random.default_rng(21)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    d[(d == 0) & (rng.random(d.shape) < 0.5)] = 900
    d[rng.random(d.shape) < 0.08] = 0
    return d.astype(np.int32)


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tau", [0, 5, 20])
@pytest.mark.parametrize("roi", [(0, 0, 0, 0), ROI])
def test_score_parity(gpu, scenario, meshes, hyps, noisy, dtype, tau, roi):
    scene = api.DeviceVector.from_host(noisy.astype(dtype).reshape(-1))
    idx = _assignments(len(hyps), len(meshes))["random"]
    got = api.score_poses_multi(meshes, idx, hyps, W, H, scenario["proj"], scene, tau, roi=roi)
    want = np.zeros(len(hyps), _lib.SCORE)
    for m in range(len(meshes)):
        sel = np.flatnonzero(idx == m)
        want[sel] = api.score_poses(meshes[m], hyps[sel], W, H, scenario["proj"], scene, tau, roi=roi)
    assert got.tobytes() == want.tobytes()
    assert got["inlier"].sum() > 0


@pytest.mark.parametrize("roi", [(0, 0, 0, 0), ROI])
def test_render_parity(gpu, scenario, meshes, hyps, roi):
    poses = hyps[:64]
    idx = _assignments(len(poses), len(meshes))["random"]
    got = api.render_multi(meshes, idx, poses, W, H, scenario["proj"], roi).to_host()
    rw, rh = (roi[2], roi[3]) if roi[2] else (W, H)
    got = got.reshape(len(poses), rh, rw)
    for m in range(len(meshes)):
        sel = np.flatnonzero(idx == m)
        want = api.render(meshes[m], poses[sel], W, H, scenario["proj"], roi).to_host().reshape(len(sel), rh, rw)
        assert np.array_equal(got[sel], want), m
    assert (got > 0).any()


# ---- edge cases ------------------------------------------------------------------------------------------------------------------
def test_mixed_mesh_sizes(gpu, scenario, gscenes, noisy):
    """A 1 M-triangle mesh (pose run 8) next to obj_06 (run 1) in one raster launch."""
    sphere = api.Model(tris=synth.uv_sphere_mesh())
    meshes = [sphere, api.Model(tris=scenario["tris"])]
    poses = synth.hypotheses(40)
    idx = (np.arange(40) % 5 != 0).astype(np.int64)              # 8 sphere, 32 obj_06 hypotheses
    got = api.refine_batch_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    _assert_refine_equal(got, _refine_single(meshes, idx, poses, gscenes["proj"]))
    sc = api.score_poses_multi(meshes, idx, poses, W, H, scenario["proj"], noisy, 5)
    for m in range(2):
        sel = np.flatnonzero(idx == m)
        assert sc[sel].tobytes() == api.score_poses(meshes[m], poses[sel], W, H, scenario["proj"], noisy, 5).tobytes()
    d = api.render_multi(meshes, idx[:10], poses[:10], W, H, scenario["proj"]).to_host().reshape(10, H, W)
    for i in range(10):
        assert np.array_equal(d[i], api.render(meshes[idx[i]], poses[i:i + 1], W, H, scenario["proj"]).to_host().reshape(H, W)), i


def test_empty_mesh_and_repeated_pointer(gpu, scenario, gscenes, noisy):
    obj = api.Model(tris=scenario["tris"])
    empty = np.zeros((0, 3, 3), np.float32)
    meshes = [obj, empty, obj.device_tris()]                      # the same buffer twice
    poses = synth.hypotheses(30)
    idx = np.arange(30) % 3
    res, sizes = api.refine_batch_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    _assert_refine_equal((res, sizes), _refine_single([obj, empty, obj], idx, poses, gscenes["proj"]))
    assert not sizes[idx == 1].any() and sizes[idx != 1].all()
    assert np.array_equal(res["T"][idx == 1], np.tile(np.eye(4, dtype=np.float32).reshape(16), (10, 1)))
    sc = api.score_poses_multi(meshes, idx, poses, W, H, scenario["proj"], noisy, 5)
    assert sc[idx == 1].tobytes() == np.zeros(10, _lib.SCORE).tobytes()
    d = api.render_multi(meshes, idx, poses, W, H, scenario["proj"]).to_host().reshape(30, H, W)
    assert not d[idx == 1].any() and d[idx == 0].any()


def test_groups_straddle_depth_chunks(gpu):
    """A frame of 2^24 pixels holds 64 hypotheses per chunk (depth_chunk): 150 hypotheses of three meshes run in three chunks, and the
    groups of the grouped batch cross the chunk boundaries."""
    rng = np.random.default_rng(8)
    Wb, Hb = 4096, 4096
    K = np.array([4.0 * Wb, 0, Wb / 2, 0, 4.0 * Wb, Hb / 2, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Wb, Hb)
    tris = [random_mesh(rng, 400, 30.0), random_mesh(rng, 250, 20.0), random_mesh(rng, 300, 25.0)]
    base = synth.hypotheses(150, seed=3)
    base[:, 2, 3] += 600.0                                         # small silhouettes in the large frame
    scene_depth = api.render_host(api.Model(tris=tris[0]), base[:1], Wb, Hb, proj)[0]
    scene = api.Scene_projective().init_Scene_projective_cuda(scene_depth, K, Wb, Hb)
    idx = np.array([0] * 50 + [1] * 50 + [2] * 50)[rng.permutation(150)]
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 3)
    res, sizes = api.refine_batch_multi(tris, idx, base, Wb, Hb, proj, K, scene, crit)
    for m in range(3):
        sel = np.flatnonzero(idx == m)
        r1, s1 = api.refine_batch(tris[m], base[sel], Wb, Hb, proj, K, scene, crit)
        assert np.array_equal(sizes[sel], s1) and res[sel].tobytes() == r1.tobytes(), m
    assert sizes.any()
    sd = api.DeviceVector.from_host(scene_depth.reshape(-1))
    sc = api.score_poses_multi(tris, idx, base, Wb, Hb, proj, sd, 10)
    for m in range(3):
        sel = np.flatnonzero(idx == m)
        assert sc[sel].tobytes() == api.score_poses(tris[m], base[sel], Wb, Hb, proj, sd, 10).tobytes(), m


def test_invalid_arguments_write_nothing(gpu, scenario, gscenes, meshes):
    lib = _lib.load()
    table, devs = api._mesh_table(meshes)
    poses = synth.hypotheses(8)
    pj, K = np.ascontiguousarray(scenario["proj"], np.float32), np.ascontiguousarray(scenario["K"], np.float32)
    d = gscenes["proj"].desc()
    for idx, n_meshes in ((np.array([0, 1, 2, 3, 4, 0, 1, 2], np.uint32), 4), (np.zeros(8, np.uint32), 0)):
        res = np.frombuffer(np.full(8 * 72, 0xA5, np.uint8).tobytes(), _lib.RESULT).copy()
        sizes = np.full(8, 0xDEADBEEF, np.uint32)
        rc = lib.pr_refine_batch_multi(table, n_meshes, idx.ctypes.data, poses.ctypes.data, 8, W, H, pj.ctypes.data, K.ctypes.data, api.SCENE_PROJ,
                                       C.addressof(d), CRIT.c(), _lib.Roi(0, 0, 0, 0), res.ctypes.data, sizes.ctypes.data)
        assert rc == _lib.PR_ERR_INVALID
        assert (res.view(np.uint8) == 0xA5).all() and (sizes == 0xDEADBEEF).all()
        sc = np.frombuffer(np.full(8 * 32, 0x5A, np.uint8).tobytes(), _lib.SCORE).copy()
        scene = api.DeviceVector.from_host(np.zeros(W * H, np.int32))
        rc = lib.pr_score_poses_multi(table, n_meshes, idx.ctypes.data, poses.ctypes.data, 8, W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0),
                                      scene.data(), 1, 5, sc.ctypes.data)
        assert rc == _lib.PR_ERR_INVALID and (sc.view(np.uint8) == 0x5A).all()
        out = api.DeviceVector.from_host(np.full(8 * W * H, 7, np.int32))
        rc = lib.pr_render_multi(table, n_meshes, idx.ctypes.data, poses.ctypes.data, 8, W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0), out.data())
        assert rc == _lib.PR_ERR_INVALID and (out.to_host() == 7).all()
    idx = np.zeros(8, np.uint32)
    rc = lib.pr_refine_batch_multi(table, 4, idx.ctypes.data, None, 8, W, H, pj.ctypes.data, K.ctypes.data, api.SCENE_PROJ,
                                   C.addressof(d), CRIT.c(), _lib.Roi(0, 0, 0, 0), res.ctypes.data, sizes.ctypes.data)
    assert rc == _lib.PR_ERR_INVALID
    assert lib.pr_refine_batch_multi(None, 0, None, None, 0, W, H, None, None, api.SCENE_PROJ, None, CRIT.c(), _lib.Roi(0, 0, 0, 0), None, None) == _lib.PR_OK
    with pytest.raises(api.PoseRefineError) as e:                 # the single-mesh ROI check
        api.score_poses_multi(meshes, np.zeros(8, np.int64), poses, W, H, scenario["proj"], np.zeros((H, W), np.int32), 5, roi=(600, 0, 100, 10))
    assert e.value.code == _lib.PR_ERR_INVALID


def test_raster_mode_does_not_apply(gpu, scenario, gscenes, meshes, hyps):
    poses = hyps[:48]
    idx = np.arange(48) % len(meshes)
    ref = api.refine_batch_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    api.set_option("raster_mode", 1)
    try:
        got = api.refine_batch_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    finally:
        api.set_option("raster_mode", 0)
    _assert_refine_equal(got, ref)


@pytest.mark.device_solve
def test_pending_slot_batch_survives(gpu, model, scenario, gscenes, meshes, hyps):
    poses = hyps[:64]
    want = api.refine_batch(model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    idx = np.arange(64) % len(meshes)
    want_multi = _refine_single(meshes, idx, poses[::-1].copy(), gscenes["nn"])
    api.refine_submit(0, model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"], CRIT)
    got_multi = api.refine_batch_multi(meshes, idx, poses[::-1].copy(), W, H, scenario["proj"], scenario["K"], gscenes["nn"], CRIT)
    got = api.refine_wait(0)
    _assert_refine_equal(got, want)
    _assert_refine_equal(got_multi, want_multi)


def test_threads_with_private_contexts(gpu, scenario, gscenes, hyps):
    host = [scenario["tris"], _rigid(scenario["tris"], -0.2, (0.0, 5.0, 0.0)), scenario["tris"] * np.float32(1.1)]
    jobs = [(hyps[:96], np.arange(96) % 3), (hyps[96:200], np.random.default_rng(4).integers(0, 3, 104))]
    want = [_refine_single(host, idx, p, gscenes["proj"]) for p, idx in jobs]
    out, errs = [None, None], []

    def run(k):
        try:
            api.thread_context(True)
            d = scenario["depth"][1]
            scene = api.Scene_projective().init_Scene_projective_cuda(d, scenario["K"])
            for _ in range(3):
                out[k] = api.refine_batch_multi(host, jobs[k][1], jobs[k][0], W, H, scenario["proj"], scenario["K"], scene, CRIT)
            api.thread_context(False)
        except Exception as e:                                    # noqa: BLE001 -- reported below
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        _assert_refine_equal(out[k], want[k])


# ---- the 32768-hypothesis launch seams of mixed batches ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_batch(gpu):
    """verify_ref.launch_split_case with two meshes (the box and a copy scaled by 0.8) in runs of five hypotheses, one of which straddles the seam;
    behind the seam every hypothesis takes the next pose (seam_cases.seam_index)."""
    c = launch_split_case()
    meshes = [c["tris"], S.small_mesh(c["tris"])]
    idx, mi = S.seam_index(S.P, 8), S.mesh_runs(S.P)
    return dict(c=c, meshes=meshes, idx=idx, mi=mi, poses=c["poses"][idx], renders=[O.render(t, c["poses"], c["W"], c["H"], c["proj"]) for t in meshes])


def test_render_batch_of_two_launches(seam_batch):
    """render_multi: fill and count run in pieces around one raster launch over all groups.  Every image is the oracle's render of its mesh and pose."""
    b, c = seam_batch, seam_batch["c"]
    per_mesh = [api.render_host(t, c["poses"], c["W"], c["H"], c["proj"]) for t in b["meshes"]]
    for m in (0, 1):
        assert np.array_equal(per_mesh[m], b["renders"][m]), m
    table, take = S.mixed_table(per_mesh, b["mi"], b["idx"])
    S.assert_seam_visible(table, take)
    got = api.render_multi(b["meshes"], b["mi"], b["poses"], c["W"], c["H"], c["proj"]).to_host().reshape(S.P, -1)
    S.seam_report("render_multi", [(r > 0).sum((1, 2)).tolist() for r in per_mesh], (got > 0).sum(1), take)
    S.assert_records_take(got, table, take)


def test_score_batch_of_two_launches(seam_batch):
    b, c = seam_batch, seam_batch["c"]
    from verify_ref import assert_scores_equal, score_ref
    per_mesh = [api.score_poses(t, c["poses"], c["W"], c["H"], c["proj"], c["scene"], c["tau"]) for t in b["meshes"]]
    for m in (0, 1):
        assert_scores_equal(per_mesh[m], score_ref(b["renders"][m], c["scene"], c["tau"]))
    table, take = S.mixed_table(per_mesh, b["mi"], b["idx"])
    S.assert_seam_visible(table, take)
    got = api.score_poses_multi(b["meshes"], b["mi"], b["poses"], c["W"], c["H"], c["proj"], c["scene"], c["tau"])
    S.seam_report("score_poses_multi", [s["visible"].tolist() for s in per_mesh], np.stack([got["visible"], got["inlier"]], 1), take)
    S.assert_records_take(got, table, take)


@pytest.mark.parametrize("solve", [api.SOLVE_HOST, pytest.param(api.SOLVE_DEVICE, marks=pytest.mark.device_solve)])
def test_refine_batch_of_two_launches(seam_batch, solve):
    b, c = seam_batch, seam_batch["c"]
    scene = S.device_scenes()["proj"]
    ppb = api.get_option("points_per_block")
    api.set_option("solve", solve)
    try:
        per_mesh = []
        for m in (0, 1):
            res, sizes = api.refine_batch(b["meshes"][m], c["poses"], c["W"], c["H"], c["proj"], S.SPLIT_K, scene, api.ICPConvergenceCriteria(*S.CRIT))
            ores, osizes = S.refine_ref("proj", ppb, small=bool(m))
            assert np.array_equal(sizes, osizes) and np.array_equal(res["fitness"], ores["fitness"]), m
            assert np.allclose(res["T"], ores["T"], rtol=0, atol=TOL_T), m
            per_mesh.append(S.refine_rows((res, sizes)))
        table, take = S.mixed_table(per_mesh, b["mi"], b["idx"])
        S.assert_seam_visible(table, take)
        got = api.refine_batch_multi(b["meshes"], b["mi"], b["poses"], c["W"], c["H"], c["proj"], S.SPLIT_K, scene, api.ICPConvergenceCriteria(*S.CRIT))
        S.seam_report(("refine_batch_multi", solve), [t[:, -4:].copy().view(np.uint32).reshape(-1).tolist() for t in per_mesh],
                      np.stack([got[1], got[0]["fitness"]], 1), take)
        S.assert_records_take(S.refine_rows(got), table, take)
    finally:
        api.set_option("solve", api.SOLVE_HOST)
