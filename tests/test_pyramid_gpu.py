"""GPU tests (-m gpu) of coarse-to-fine refinement (pr_refine_pyramid / pr_refine_pyramid_multi): every level's cloud size and record and the
final record against the reference composed from the CPU oracle (tests/pyramid_ref.py), and byte for byte against refine_batch, against
other compositions of the same batch and against the single-mesh call."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pyramid_ref as R
import seam_cases as S
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H, TOL_T, inliers
from test_nn_exact_gpu import options
from verify_ref import launch_split_case

pytestmark = pytest.mark.gpu

TABLES = {
    "default": api.PYRAMID_DEFAULT,
    "odd": ((8, (0, 0, 4)), (3, (0, 0, 3)), (1, (1e-5, 1e-5, 30))),        # a stride that is no power of two, and an early exit
}
_ref_cache = {}


def _ref(scenario, key, poses, kind, levels, roi=(0, 0, 0, 0)):
    """The composed reference; the same for both solve modes, so computed once per case."""
    k = (key, kind, roi, api.get_option("points_per_block"))
    if k not in _ref_cache:
        scene = scenario["proj_scene" if kind == "proj" else "nn_scene"]
        _ref_cache[k] = R.refine_pyramid(scenario["tris"], poses, W, H, scenario["proj"], scenario["K"], scene, levels, k[3], roi)
    return _ref_cache[k]


def _assert_records(got, want, sizes, what):
    assert np.array_equal(got["fitness"], want["fitness"]), what
    assert np.array_equal(inliers(got["fitness"], sizes), inliers(want["fitness"], sizes)), what
    assert np.allclose(got["inlier_rmse"], want["inlier_rmse"], rtol=1e-6, atol=0), what
    assert np.allclose(got["T"], want["T"], rtol=0, atol=TOL_T), what


def _assert_against_ref(got, want, what=""):
    res, lres, lsizes = got
    ores, olres, olsizes = want
    assert np.array_equal(lsizes, olsizes), what
    for l in range(len(lsizes)):
        _assert_records(lres[l], olres[l], lsizes[l], (what, "level", l))
    _assert_records(res, ores, lsizes[-1], (what, "final"))
    assert res["fitness"].tobytes() == lres[-1]["fitness"].tobytes() and res["inlier_rmse"].tobytes() == lres[-1]["inlier_rmse"].tobytes(), what


def _pyr(model, poses, scenario, scene, levels, roi=None, return_levels=True):
    return api.refine_pyramid(model, poses, W, H, scenario["proj"], scenario["K"], scene, levels, roi=roi, return_levels=return_levels)


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1: against the composed reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("kind,P", [("proj", 24), ("nn", 6)])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_pyramid_against_reference(gpu, model, scenario, gscenes, solve, kind, P, table):
    api.set_option("solve", solve)
    try:
        poses = synth.hypotheses(P)
        got = _pyr(model, poses, scenario, gscenes[kind], TABLES[table])
        want = _ref(scenario, ("t1", table, P), poses, kind, TABLES[table])
        _assert_against_ref(got, want, (solve, kind, table))
        assert (got[2][0] > 0).all() and (got[2][0] < got[2][-1]).all()       # every level saw its cloud, the coarse one a thinner cloud
        # the plain return value: the stride-1 cloud size, as refine_batch returns it
        res2, sizes = _pyr(model, poses, scenario, gscenes[kind], TABLES[table], return_levels=False)
        assert res2.tobytes() == got[0].tobytes() and np.array_equal(sizes, got[2][-1])
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- 2: one level of stride 1 is refine_batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi", [None, (160, 80, 320, 240)])
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_one_full_level_equals_refine_batch(gpu, model, scenario, gscenes, solve, kind, roi):
    api.set_option("solve", solve)
    try:
        poses = synth.hypotheses(24 if kind == "proj" else 6)
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 8)
        want, wsizes = api.refine_batch(model, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], crit, roi=roi)
        res, lres, lsizes = _pyr(model, poses, scenario, gscenes[kind], [api.PyramidLevel(1, crit)], roi=roi)
        assert np.array_equal(lsizes[0], wsizes) and wsizes.min() > 0
        assert res.tobytes() == want.tobytes() and lres[0].tobytes() == want.tobytes()
        res2, sizes2 = _pyr(model, poses, scenario, gscenes[kind], [(1, (0.0, 0.0, 8))], roi=roi, return_levels=False)
        assert res2.tobytes() == want.tobytes() and np.array_equal(sizes2, wsizes)
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- 3: the grid is anchored on the frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_roi_that_contains_every_silhouette_equals_full_frame(gpu, model, scenario, gscenes, solve):
    api.set_option("solve", solve)
    try:
        poses = synth.hypotheses(16)
        depth = O.render(scenario["tris"], poses, W, H, scenario["proj"])
        ys, xs = np.nonzero(depth.max(axis=0))
        x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
        x0 -= (x0 + 1) % 2; y0 -= (y0 + 1) % 2                       # the origin moved to odd coordinates (still containing every silhouette)
        assert x0 % 2 == 1 and y0 % 2 == 1 and x0 > 0 and y0 > 0
        roi = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
        for table in sorted(TABLES):
            full = _pyr(model, poses, scenario, gscenes["proj"], TABLES[table])
            crop = _pyr(model, poses, scenario, gscenes["proj"], TABLES[table], roi=roi)
            assert _same_bytes(full, crop), table
    finally:
        api.set_option("solve", api.SOLVE_HOST)


@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_cutting_roi_with_odd_origin_against_reference(gpu, model, scenario, gscenes, solve):
    api.set_option("solve", solve)
    try:
        roi = (161, 81, 320, 240)
        poses = synth.hypotheses(8)
        for table in sorted(TABLES):
            got = _pyr(model, poses, scenario, gscenes["proj"], TABLES[table], roi=roi)
            want = _ref(scenario, ("t3", table), poses, "proj", TABLES[table], roi)
            _assert_against_ref(got, want, (solve, table))
            assert not np.array_equal(got[2], _pyr(model, poses, scenario, gscenes["proj"], TABLES[table])[2])      # the window does cut
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- 4: a hypothesis' result does not depend on the batch around it --------------------------------------------------------------
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_full_batch_permutation_and_single_poses(gpu, model, scenario, gscenes, solve):
    api.set_option("solve", solve)
    try:
        P = 256
        poses = synth.hypotheses(P)
        got = _pyr(model, poses, scenario, gscenes["proj"], api.PYRAMID_DEFAULT)
        perm = np.random.default_rng(3).permutation(P)
        got_p = _pyr(model, poses[perm], scenario, gscenes["proj"], api.PYRAMID_DEFAULT)
        assert _same_bytes((got[0][perm], got[1][:, perm], got[2][:, perm]), got_p)
        for i in (0, 17, 255):
            one = _pyr(model, poses[i:i + 1], scenario, gscenes["proj"], api.PYRAMID_DEFAULT)
            assert _same_bytes((got[0][i:i + 1], got[1][:, i:i + 1], got[2][:, i:i + 1]), one), i
    finally:
        api.set_option("solve", api.SOLVE_HOST)


@pytest.mark.device_solve
def test_batch_spanning_two_depth_chunks_equals_its_halves(gpu, model, scenario, gscenes):
    """The synchronous path renders a batch in chunks of about 4 GiB of depth workspace (3495 frames of 640 x 480): 3600 hypotheses are two."""
    P = 3600
    assert P > (4 << 30) // (W * H * 4)
    poses = synth.hypotheses(P)
    levels = ((4, (0, 0, 2)), (1, (0, 0, 1)))
    got = _pyr(model, poses, scenario, gscenes["proj"], levels)
    a = _pyr(model, poses[:P // 2], scenario, gscenes["proj"], levels)
    b = _pyr(model, poses[P // 2:], scenario, gscenes["proj"], levels)
    assert _same_bytes(got, (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]], axis=1), np.concatenate([a[2], b[2]], axis=1)))


# ---- 5: mixed batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_multi_equals_one_call_per_mesh(gpu, scenario, gscenes, solve, kind):
    t = scenario["tris"]
    meshes = [api.Model(tris=t), np.ascontiguousarray(t * np.float32(0.8)), api.DeviceVector.from_host(np.ascontiguousarray(t * np.float32(1.1)).reshape(-1))]
    P = 48 if kind == "proj" else 9
    poses = synth.hypotheses(P)
    idx = np.random.default_rng(7).integers(0, 3, P)
    api.set_option("solve", solve)
    try:
        for roi in (None, (161, 81, 320, 240)):
            got = api.refine_pyramid_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], TABLES["odd"], roi=roi, return_levels=True)
            res = np.zeros(P, _lib.RESULT); lres = np.zeros((3, P), _lib.RESULT); lsizes = np.zeros((3, P), np.uint32)
            for m in range(3):
                sel = np.flatnonzero(idx == m)
                assert len(sel)
                res[sel], lres[:, sel], lsizes[:, sel] = _pyr(meshes[m], poses[sel], scenario, gscenes[kind], TABLES["odd"], roi=roi)
            assert _same_bytes(got, (res, lres, lsizes)), roi
            plain = api.refine_pyramid_multi(meshes, idx, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], TABLES["odd"], roi=roi)
            assert plain[0].tobytes() == res.tobytes() and np.array_equal(plain[1], lsizes[-1])
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- 6: edges --------------------------------------------------------------------------------------------------------------------
def _misses_grid16(tris, pose, scenario):
    ys, xs = np.nonzero(O.render(tris, pose[None], W, H, scenario["proj"])[0] > 0)
    return len(xs) > 20 and not ((xs % 16 == 0) & (ys % 16 == 0)).any() and ((xs % 4 == 0) & (ys % 4 == 0)).any()


def _pose_between_grid_points(tris, base, scenario, reach, step):
    """`base` shifted in x / y until the silhouette lies between the points of the stride-16 grid (and on some of the stride-4 grid): found
    with the oracle's render.  Then the same pose moved by a few millimetres that still misses the grid: (scene pose, hypothesis)."""
    for dy in range(0, reach, step):
        for dx in range(0, reach, step):
            p = base.copy(); p[0, 3] += dx; p[1, 3] += dy
            if not _misses_grid16(tris, p, scenario):
                continue
            for k in (1.0, -1.0, 0.5, -0.5):
                q = p.copy(); q[0, 3] += k * step * 0.5; q[2, 3] += k * step
                if _misses_grid16(tris, q, scenario):
                    return p, q
    raise AssertionError("no such pose")


@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_empty_levels_and_zero_iterations(gpu, model, scenario, solve):
    """obj_06 4 m away is a 14-pixel silhouette that fits between the points of the stride-16 grid: that level is empty, the later ones run.
    (The reference's scene normals are zero that far out, so the later levels score without moving anything; a 0.12-scale copy at 700 mm is
    as small in the image, has normals, and does move.)  With them a pose that renders nothing, and a middle level of no iterations."""
    tris = scenario["tris"]
    base = synth.scene_pose().copy(); base[0, 3] += 1500.0; base[2, 3] = 4000.0
    far, hyp = _pose_between_grid_points(tris, base, scenario, 160, 5)
    small = np.ascontiguousarray(tris * np.float32(0.12))
    base = synth.scene_pose().copy(); base[0, 3] += 150.0; base[2, 3] = 700.0
    near, hyp_small = _pose_between_grid_points(small, base, scenario, 40, 2)
    scene_depth = scenario["depth"][1].copy()
    for t, p in ((tris, far), (small, near)):
        d = O.render(t, p[None], W, H, scenario["proj"])[0]
        free = (d > 0) & (scene_depth == 0)
        scene_depth[free] = d[free]
    gone = synth.scene_pose().copy(); gone[0, 3] += 4000.0                # renders nothing
    poses = np.concatenate([synth.hypotheses(3), hyp[None], gone[None]])
    levels = ((16, (0, 0, 3)), (4, (0, 0, 0)), (1, (0, 0, 3)))          # the middle level only scores
    gs = api.Scene_projective().init_Scene_projective_cuda(scene_depth, scenario["K"])
    osc = O.ProjScene(scene_depth, scenario["K"])
    ppb = api.get_option("points_per_block")
    eye = np.eye(4, dtype=np.float32).reshape(16)
    api.set_option("solve", solve)
    try:
        got = api.refine_pyramid(model, poses, W, H, scenario["proj"], scenario["K"], gs, levels, return_levels=True)
        want = R.refine_pyramid(tris, poses, W, H, scenario["proj"], scenario["K"], osc, levels, ppb)
        _assert_against_ref(got, want, solve)
        res, lres, lsizes = got
        # the far hypothesis: nothing on the stride-16 grid -> the untouched record there, and the later levels still run
        assert lsizes[0, 3] == 0 and lsizes[1, 3] > 0 and lsizes[2, 3] > lsizes[1, 3]
        assert np.array_equal(lres[0, 3]["T"], eye) and lres[0, 3]["fitness"] == 0 and lres[0, 3]["inlier_rmse"] == 0
        assert lres[1, 3]["fitness"] > 0 and lres[2, 3]["fitness"] > 0
        # a level with max_iteration = 0 scores and leaves the transform alone
        assert all(np.array_equal(lres[1, i]["T"], eye) for i in range(5)) and (lres[1, :4]["fitness"] > 0).all()
        assert not any(np.array_equal(lres[0, i]["T"], eye) or np.array_equal(lres[2, i]["T"], eye) for i in range(3))
        # the pose that renders nothing: empty at every level, identity / 0 / 0 throughout
        assert not lsizes[:, 4].any() and np.array_equal(res[4]["T"], eye) and res[4]["fitness"] == 0 and res[4]["inlier_rmse"] == 0
        assert all(np.array_equal(lres[l, 4]["T"], eye) for l in range(3))
        alone = api.refine_pyramid(model, gone[None], W, H, scenario["proj"], scenario["K"], gs, levels, return_levels=True)
        assert _same_bytes(alone, (res[4:5], lres[:, 4:5], lsizes[:, 4:5]))
        # the small copy: empty at stride 16, refined by the last level from the identity the empty level left
        got = api.refine_pyramid(api.Model(tris=small), hyp_small[None], W, H, scenario["proj"], scenario["K"], gs, levels, return_levels=True)
        want = R.refine_pyramid(small, hyp_small[None], W, H, scenario["proj"], scenario["K"], osc, levels, ppb)
        _assert_against_ref(got, want, (solve, "small"))
        res, lres, lsizes = got
        assert lsizes[0, 0] == 0 and lsizes[2, 0] > lsizes[1, 0] > 0 and np.array_equal(lres[0, 0]["T"], eye)
        assert lres[2, 0]["fitness"] > 0 and not np.array_equal(res[0]["T"], eye) and np.array_equal(res[0]["T"], lres[2, 0]["T"])
    finally:
        api.set_option("solve", api.SOLVE_HOST)


def test_no_poses_and_invalid_arguments(gpu, model, scenario, gscenes):
    e0 = np.zeros((0, 16), np.float32)
    res, lres, lsizes = _pyr(model, e0, scenario, gscenes["proj"], api.PYRAMID_DEFAULT)
    assert len(res) == 0 and lres.shape == (3, 0) and lsizes.shape == (3, 0)
    res, sizes = api.refine_pyramid_multi([model], np.zeros(0, np.int64), e0, W, H, scenario["proj"], scenario["K"], gscenes["proj"])
    assert len(res) == 0 and len(sizes) == 0
    lib = _lib.load()
    poses = synth.hypotheses(2)
    td = model.device_tris()
    d = gscenes["proj"].desc()
    pj, k = np.ascontiguousarray(scenario["proj"], np.float32).reshape(-1), np.ascontiguousarray(scenario["K"], np.float32).reshape(-1)
    good = (_lib.PyramidLevel * 2)(api.PyramidLevel(2, (0, 0, 2)), api.PyramidLevel(1, (0, 0, 2)))

    def call(levels=good, n_levels=2, roi=(0, 0, 0, 0), width=W, height=H, out=True, poses_p=poses.ctypes.data, scene=C.addressof(d), tris=td.data()):
        res = np.full(2 * 72, 7, np.uint8); lres = np.full(4 * 2 * 72, 7, np.uint8); lsz = np.full(8, 0x07070707, np.uint32)
        rc = lib.pr_refine_pyramid(tris, td.size() // 9, poses_p, 2, width, height, pj.ctypes.data, k.ctypes.data, _lib.SCENE_PROJ, scene, levels, n_levels,
                                   _lib.Roi(*roi), res.ctypes.data if out else None, lres.ctypes.data, lsz.ctypes.data)
        assert (res == 7).all() and (lres == 7).all() and (lsz == 0x07070707).all()        # nothing written
        return rc

    def table(*lv):
        return (_lib.PyramidLevel * len(lv))(*[api.PyramidLevel(*x) for x in lv])

    bad = dict(no_levels=dict(n_levels=0), five_levels=dict(levels=table(*[(1, (0, 0, 1))] * 5), n_levels=5),
               stride_0=dict(levels=table((0, (0, 0, 1)), (1, (0, 0, 1)))), stride_17=dict(levels=table((1, (0, 0, 1)), (17, (0, 0, 1)))),
               negative_iterations=dict(levels=table((2, (0, 0, -1)), (1, (0, 0, 1)))), null_levels=dict(levels=None), null_results=dict(out=False),
               roi_outside=dict(roi=(600, 0, 100, 100)), frame_too_large=dict(width=8193), zero_frame=dict(height=0), null_poses=dict(poses_p=None),
               null_scene=dict(scene=None), null_mesh=dict(tris=None))
    for what, kw in bad.items():
        assert call(**kw) == _lib.PR_ERR_INVALID, what
    with pytest.raises(api.PoseRefineError) as e:
        _pyr(model, poses, scenario, gscenes["proj"], [(32, (0, 0, 1))])
    assert e.value.code == _lib.PR_ERR_INVALID and "stride" in str(e.value)
    # the mesh index of a mixed batch
    mesh = (_lib.MeshRef * 1)(_lib.MeshRef(td.data(), td.size() // 9))
    idx = np.array([0, 1], np.uint32)
    res = np.full(2 * 72, 7, np.uint8)
    assert lib.pr_refine_pyramid_multi(mesh, 1, idx.ctypes.data, poses.ctypes.data, 2, W, H, pj.ctypes.data, k.ctypes.data, _lib.SCENE_PROJ, C.addressof(d), good, 2,
                                       _lib.Roi(0, 0, 0, 0), res.ctypes.data, None, None) == _lib.PR_ERR_INVALID
    assert (res == 7).all()
    # and the library is fine afterwards
    out = _pyr(model, poses, scenario, gscenes["proj"], [(2, (0, 0, 2)), (1, (0, 0, 2))])
    assert (out[2] > 0).all()


# ---- 7: nothing leaks into the existing path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_refine_batch_is_unchanged_by_pyramid_calls(gpu, model, scenario, gscenes, solve, kind):
    api.set_option("solve", solve)
    try:
        poses = synth.hypotheses(32 if kind == "proj" else 6)
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 10)
        before = api.refine_batch(model, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], crit)
        for table in sorted(TABLES):
            _pyr(model, poses, scenario, gscenes[kind], TABLES[table])
            _pyr(model, poses, scenario, gscenes[kind], TABLES[table], roi=(161, 81, 320, 240))
        after = api.refine_batch(model, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], crit)
        assert _same_bytes(before, after)
        api.refine_submit(0, model, poses, W, H, scenario["proj"], scenario["K"], gscenes[kind], crit)
        mid = _pyr(model, poses, scenario, gscenes[kind], api.PYRAMID_DEFAULT)     # with a batch pending on a slot
        assert _same_bytes(api.refine_wait(0), before)
        assert _same_bytes(mid, _pyr(model, poses, scenario, gscenes[kind], api.PYRAMID_DEFAULT))
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- 8: the 32768-hypothesis launch seams ----------------------------------------------------------------------------------------
def _split_pyr(c, tris, poses, scene, levels):
    return api.refine_pyramid(tris, poses, c["W"], c["H"], c["proj"], S.SPLIT_K, scene, levels, return_levels=True)


def _eight_against_ref(c, kind, levels, what, small=False):
    """The eight-hypothesis call on the split case, held to pyramid_ref by this file's rule; returned as one row of bytes per hypothesis."""
    tris = S.small_mesh(c["tris"]) if small else c["tris"]
    eight = _split_pyr(c, tris, c["poses"], S.device_scenes()[kind], levels)
    _assert_against_ref(eight, S.pyramid_ref_records(kind, tuple(levels), api.get_option("points_per_block"), small), what)
    return eight, S.pyramid_rows(eight)


SOLVES = [api.SOLVE_HOST, pytest.param(api.SOLVE_DEVICE, marks=pytest.mark.device_solve)]


@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("solve", SOLVES)
def test_batch_of_two_launches(gpu, solve, kind):
    """32768 + 5 hypotheses of verify_ref.launch_split_case, two levels: the count and emit launches run in two pieces, and the level loops
    (host and device solve) over more than 32768 clouds.  Behind the seam every hypothesis takes the next pose (seam_cases.seam_index); every
    hypothesis' whole output -- record, level records, level sizes -- is that of its pose in the eight-hypothesis call, byte for byte."""
    c = launch_split_case()
    api.set_option("solve", solve)
    try:
        eight, rows8 = _eight_against_ref(c, kind, S.PYR2, (solve, kind))
        idx = S.seam_index(S.P, 8)
        S.assert_seam_visible(rows8, idx)
        # the level loops cut a batch into pose groups (two by default) and launch the pass per group: one group (pose_groups 1) puts all 32773
        # hypotheses on one pass launch, which then runs in two pieces itself; the count, scan and emit launches cross their seams either way
        for groups in (1, 0):
            with options(pose_groups=groups):
                got = _split_pyr(c, c["tris"], c["poses"][idx], S.device_scenes()[kind], S.PYR2)
            S.seam_report(("pyramid", solve, kind, "pose_groups", groups), eight[2], got[2].T, idx)
            S.assert_records_take(S.pyramid_rows(got), rows8, idx)
    finally:
        api.set_option("solve", api.SOLVE_HOST)


@pytest.mark.parametrize("solve,kind", [(api.SOLVE_HOST, "proj"), pytest.param(api.SOLVE_DEVICE, "nn", marks=pytest.mark.device_solve)])
def test_row_scan_of_two_launches(gpu, solve, kind):
    """8200 hypotheses x 4 levels: the row scan runs over 32800 (level, hypothesis) images in two pieces, the second of which starts at
    hypothesis 8168 of the last level; the count and emit launches are single.  The index steps there, so neighbours across the seam differ."""
    c = launch_split_case()
    api.set_option("solve", solve)
    try:
        eight, rows8 = _eight_against_ref(c, kind, S.PYR4, (solve, kind, "scan"))
        idx = S.seam_index(S.SCAN_P, 8, S.SCAN_SEAM)
        assert len(S.PYR4) * S.SCAN_P > S.SEAM == 3 * S.SCAN_P + S.SCAN_SEAM
        S.assert_seam_visible(rows8, idx, S.SCAN_SEAM)
        got = _split_pyr(c, c["tris"], c["poses"][idx], S.device_scenes()[kind], S.PYR4)
        S.seam_report(("row scan", solve, kind), eight[2], got[2].T, idx, S.SCAN_SEAM)
        S.assert_records_take(S.pyramid_rows(got), rows8, idx, S.SCAN_SEAM)
    finally:
        api.set_option("solve", api.SOLVE_HOST)


@pytest.mark.parametrize("solve", SOLVES)
def test_mixed_batch_of_two_launches(gpu, solve):
    """32768 + 5 hypotheses of two meshes (the box and a copy scaled by 0.8) in runs of five, one of which straddles the seam: every hypothesis'
    whole output is that of its pose in the eight-hypothesis single-mesh call of its mesh."""
    c = launch_split_case()
    meshes = [c["tris"], S.small_mesh(c["tris"])]
    api.set_option("solve", solve)
    try:
        per_mesh = [_eight_against_ref(c, "proj", S.PYR2, (solve, "mesh", m), small=bool(m)) for m in (0, 1)]
        idx, mi = S.seam_index(S.P, 8), S.mesh_runs(S.P)
        table, take = S.mixed_table([rows for _, rows in per_mesh], mi, idx)
        S.assert_seam_visible(table, take)
        got = api.refine_pyramid_multi(meshes, mi, c["poses"][idx], c["W"], c["H"], c["proj"], S.SPLIT_K, S.device_scenes()["proj"], S.PYR2, return_levels=True)
        S.seam_report(("mixed pyramid", solve), [e[2][-1].tolist() for e, _ in per_mesh], got[2].T, take)
        S.assert_records_take(S.pyramid_rows(got), table, take)
    finally:
        api.set_option("solve", api.SOLVE_HOST)
