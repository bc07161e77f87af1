"""GPU tests (-m gpu) of the box raster and of everything that consumes the boxes, on the hard batches of tests/box_stress.py: strong
perspective, every frame border, exotic intrinsics, mesh coordinates far from the origin, whole-frame, few-pixel and empty boxes packed in
one batch.  Everything is held to R, the oracle's FULL-FRAME renders of the batch (oracle_lib.render knows no boxes), never to another route
of the library: the box image itself (compose_detections' front depth of one hypothesis is its packed box unpacked into the frame), the
scoring kinds that walk the boxes, the fused refine path synchronously and on the slots with loose and tight boxes, mixed batches and the
pyramid; then the kernels that combine TWO boxes (VSD over the union, interpenetration over the intersection and in LDS bands, the overlap
matrix), the span render's far plane, the contour fit and the fused information pass.  A pixel box that is one pixel too small, or a
packed-box address that is off, faults nothing: it changes a count here."""
import numpy as np
import pytest

import contour_fit_ref as CF
import info_ref
import oracle_lib as O
import pyramid_ref
from box_stress import (FIT_TJR, FIT_TJR_WIDE, H, NONE, ROIS, SLACKS, TAU, VSD_DELTA, W, drawn_count, fit_reference, interleaved, model_centres, nearest_map,
                        one_truths, pair_records, returned_planes, roi_renders, span_planes, stress_batches, vsd_pairing, vsd_reference)
from compose_ref import Composite, assert_composites_equal, check_invariants, compose_ref
from contour_ref import assert_contours_equal, contour_ref, edge_distance_ref
from cover_ref import KEEP_ALL, assert_cover_equal, cover_ref, supports_of
from gpu_common import TOL_T, inliers
from normals_ref import assert_identities, assert_normals_equal, normals_ref
from pose_refine_amd import api
from select_ref import overlap_ref
from solid_ref import check_invariants as check_pair_invariants, pairs_ref, span_ref_multi
from test_contour_fit_gpu import assert_records
from test_information_gpu import Kit, assert_record
from test_select_gpu import _assert_overlap
from test_tight_box_gpu import same, tight_batches
from verify_ref import assert_scores_equal, score_ref
from vsd_ref import SMALL_TAUS, assert_vsd_equal, vsd_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.int32, np.uint16]
CRITS = [(0.0, 0.0, 1), (0.0, 0.0, 4)]


@pytest.fixture(scope="module")
def batches():
    return stress_batches()


@pytest.fixture(scope="module")
def models(gpu, batches):
    """One api.Model per batch (every offset mesh is its own), resident on the device for the module."""
    return [api.Model(tris=b["tris"]) for b in batches]


def _scene(b, dtype):
    assert b["scene"].min() >= 0 and b["scene"].max() < 2**16
    return np.ascontiguousarray(b["scene"].astype(dtype))


def _drawn(b):
    return drawn_count(b["R"])


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _score_ref(k, b, roi=NONE):
    """(renders, reference scores) of batch k inside `roi`; the same for both scene types, whose values fit uint16."""
    r = b["R"] if roi == NONE else roi_renders(k, roi)
    return r, _cached(("score", k, roi), lambda: score_ref(r, b["scene"], TAU, roi))


# ---- the box image itself -----------------------------------------------------------------------------------------------------------------
def test_each_hypothesis_alone_is_its_full_frame_render(gpu, batches, models):
    """One hypothesis composed alone: the front depth IS its packed box unpacked into the frame, and must be the oracle's render pixel for pixel."""
    for b, m in zip(batches, models):
        sd = api.DeviceVector.from_host(b["scene"].reshape(-1))
        for i in range(len(b["poses"])):
            labels, depth, sc, vis, frame = api.compose_detections(m, b["poses"][i:i + 1], W, H, b["proj"], sd, TAU)
            got = depth.to_host().reshape(H, W)
            want = np.maximum(b["R"][i], 0)                       # R[i] itself, but for fragments behind the camera (box_stress.drawn_count)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (b["name"], i, b["families"][i], len(bad), bad[:5], got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
            assert np.array_equal(labels.to_host().reshape(H, W) == 0, want > 0)
            assert sc["visible"][0] == vis["owned"][0] == frame["covered"] == np.count_nonzero(want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_composed_batch(gpu, batches, models, dtype):
    for k, (b, m) in enumerate(zip(batches, models)):
        scene = _scene(b, dtype)
        want = _cached(("compose", k), lambda: compose_ref(b["R"], b["scene"], TAU))
        labels, depth, sc, vis, frame = api.compose_detections(m, b["poses"], W, H, b["proj"], scene, TAU)
        got = Composite(labels.to_host().reshape(H, W), depth.to_host().reshape(H, W), vis, frame, None)
        assert_composites_equal(got, want)
        check_invariants(got, sc)
        assert_scores_equal(sc, _score_ref(k, b)[1])
        for roi in ROIS:
            r = roi_renders(k, roi)
            labels, depth, sc, vis, frame = api.compose_detections(m, b["poses"], W, H, b["proj"], scene, TAU, roi=roi)
            assert_composites_equal(Composite(labels.to_host().reshape(H, W), depth.to_host().reshape(H, W), vis, frame, None),
                                    _cached(("compose", k, roi), lambda: compose_ref(r, b["scene"], TAU, roi)))


# ---- scores ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("roi", [NONE] + ROIS)
def test_score_poses(gpu, batches, models, roi, dtype):
    """Byte for byte the reference's records; `visible` is the count of drawn pixels, which a clipped pixel would break."""
    for k, (b, m) in enumerate(zip(batches, models)):
        r, want = _score_ref(k, b, roi)
        got = api.score_poses(m, b["poses"], W, H, b["proj"], _scene(b, dtype), TAU, roi=roi)
        assert_scores_equal(got, want)
        assert got.tobytes() == want.tobytes(), b["name"]
        assert np.array_equal(got["visible"], drawn_count(r)), b["name"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("step", [1, 4])
def test_score_normals(gpu, batches, models, step, dtype):
    jump, cos_min = 20, float(np.cos(np.deg2rad(30.0)))
    tested = 0
    for k, (b, m) in enumerate(zip(batches, models)):
        want = _cached(("normals", k, step), lambda: normals_ref(b["R"], b["scene"], TAU, b["K"], step, jump, cos_min))
        sc, got = api.score_normals(m, b["poses"], W, H, b["proj"], _scene(b, dtype), TAU, b["K"], step, jump, cos_min)
        assert_normals_equal(got, want)
        assert_scores_equal(sc, _score_ref(k, b)[1])
        assert_identities(got, sc)
        tested += int(want["tested"].sum())
    assert tested > 1000
    k, b, m, roi = 0, batches[0], models[0], ROIS[0]              # ... and a window that cuts the silhouettes: neighbours leave the box and the window
    sc, got = api.score_normals(m, b["poses"], W, H, b["proj"], _scene(b, dtype), TAU, b["K"], step, jump, cos_min, roi=roi)
    assert_normals_equal(got, _cached(("normals", k, step, roi), lambda: normals_ref(roi_renders(k, roi), b["scene"], TAU, b["K"], step, jump, cos_min, roi)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_contours(gpu, batches, models, dtype):
    jump, radius = 10, 2
    contour = 0
    for k, (b, m) in enumerate(zip(batches, models)):
        scene = _scene(b, dtype)
        D = _cached(("edge", k), lambda: edge_distance_ref(b["scene"], jump, radius))
        ed = api.scene_edge_distance(scene, W, H, jump, radius)
        assert np.array_equal(ed.to_host().reshape(H, W), D)
        for roi in [NONE] + ROIS[1:]:
            r, want_sc = _score_ref(k, b, roi)
            want = _cached(("contour", k, roi), lambda: contour_ref(r, b["scene"], TAU, jump, D, roi))
            sc, got = api.score_contours(m, b["poses"], W, H, b["proj"], scene, TAU, jump, ed, roi=roi)
            assert_contours_equal(got, want)
            assert_scores_equal(sc, want_sc)
            contour += int(want["contour"].sum())
    assert contour > 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_cover(gpu, batches, models, dtype):
    for k, (b, m) in enumerate(zip(batches, models)):
        scene = _scene(b, dtype)
        for roi in [NONE] + ROIS[:1]:
            r, want_sc = _score_ref(k, b, roi)
            sup, n = _cached(("support", k, roi), lambda: supports_of(r, b["scene"], TAU, roi))
            for order in (api.rank_hypotheses(want_sc), np.arange(len(r))[::-1]):
                sc, cov, frame, sel = api.score_cover(m, b["poses"], W, H, b["proj"], scene, TAU, order, (1, 4), 1, None, roi=roi)
                assert_scores_equal(sc, want_sc)
                assert_cover_equal((cov, frame, sel), cover_ref(sup, n, order, 1, 4, 1, KEEP_ALL))


# ---- the fused path -------------------------------------------------------------------------------------------------------------------------
def _scenes(k, b, kind, dtype=np.int32):
    """(the library's scene, the oracle's) of batch k, made once per module."""
    def make():
        d = _scene(b, dtype)
        if kind == "proj":
            return api.Scene_projective().init_Scene_projective_cuda(d, b["K"], W, H), O.ProjScene(d, b["K"])
        return api.Scene_nn().init_Scene_nn_cuda(d, b["K"]), O.NNScene(d, b["K"])
    return _cached(("scene", k, kind, np.dtype(dtype).name), make)


def _oracle_refine(k, b, kind, crit, dtype=np.int32):
    ppb = api.get_option("points_per_block")
    return _cached(("refine", k, kind, crit, np.dtype(dtype).name, ppb),
                   lambda: O.refine_batch(b["tris"], b["poses"], W, H, b["proj"], b["K"], _scenes(k, b, kind, dtype)[1], crit, O.SUM_CANONICAL, ppb)[:2])


def _assert_refined(got, want, b, what):
    (res, sizes), (ores, osizes) = got, want
    assert np.array_equal(sizes, _drawn(b)), (what, np.flatnonzero(sizes != _drawn(b))[:10])
    assert np.array_equal(sizes, osizes), what
    worst = float(np.abs(res["T"].astype(np.float64) - ores["T"].astype(np.float64)).max()) if len(res) else 0.0
    print(f"{what}: max |T - T_oracle| = {worst:.3g}, fitness differs at {np.flatnonzero(res['fitness'] != ores['fitness']).tolist()}")
    assert np.array_equal(res["fitness"], ores["fitness"]), what
    assert np.allclose(res["T"], ores["T"], rtol=0, atol=TOL_T), (what, worst)


@pytest.mark.parametrize("raster_mode", [0, 1])
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_refine_batch(gpu, batches, models, kind, solve, raster_mode):
    """Cloud sizes are the counts of drawn pixels; fitness and transforms the oracle's, at the project's bars.  With the solve on the device
    and raster_mode 0 the call runs on a slot; profile = 1 runs the same batch through the synchronous path, which must give the same bytes."""
    api.set_option("solve", solve)
    api.set_option("raster_mode", raster_mode)
    try:
        for k, (b, m) in enumerate(zip(batches, models)):
            gs = _scenes(k, b, kind)[0]
            for crit in CRITS:
                got = api.refine_batch(m, b["poses"], W, H, b["proj"], b["K"], gs, api.ICPConvergenceCriteria(*crit))
                _assert_refined(got, _oracle_refine(k, b, kind, crit), b, (b["name"], kind, solve, raster_mode, crit))
                if solve == api.SOLVE_DEVICE and raster_mode == 0:
                    api.set_option("profile", 1)
                    try:
                        sync = api.refine_batch(m, b["poses"], W, H, b["proj"], b["K"], gs, api.ICPConvergenceCriteria(*crit))
                    finally:
                        api.set_option("profile", 0)
                    assert same(sync, got), (b["name"], kind, crit)
    finally:
        api.set_option("profile", 0)
        api.set_option("raster_mode", 0)
        api.set_option("solve", api.SOLVE_HOST)


def test_refine_batch_uint16_scene(gpu, batches, models):
    api.set_option("solve", api.SOLVE_DEVICE)
    try:
        for k, (b, m) in enumerate(zip(batches, models)):
            for kind in ("proj", "nn"):
                gs = _scenes(k, b, kind, np.uint16)[0]
                got = api.refine_batch(m, b["poses"], W, H, b["proj"], b["K"], gs, api.ICPConvergenceCriteria(*CRITS[1]))
                _assert_refined(got, _oracle_refine(k, b, kind, CRITS[1], np.uint16), b, (b["name"], kind, "uint16"))
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- the slots: loose boxes, then tight ones ------------------------------------------------------------------------------------------------
def _slot(slot, m, b, gs, crit):
    api.refine_submit(slot, m, b["poses"], W, H, b["proj"], b["K"], gs, crit)
    return api.refine_wait(slot)


def _loose_then_tight(m, b, gs, crit):
    """As test_tight_box_gpu.loose_and_tight_match, on this module's frame and against the synchronous call: two batches with tight_box = 0
    (the vertex list is made on a buffer's second batch), then one per slot with tight_box = 1; the counter advances for exactly those."""
    api.set_option("profile", 1)
    try:
        ref = api.refine_batch(m, b["poses"], W, H, b["proj"], b["K"], gs, crit)
    finally:
        api.set_option("profile", 0)
    assert np.array_equal(ref[1], _drawn(b)), b["name"]
    try:
        api.set_option("tight_box", 0)
        before = tight_batches()
        for slot in (0, 1):
            assert same(_slot(slot, m, b, gs, crit), ref), (b["name"], "tight_box=0", slot)
        assert tight_batches() == before
        api.set_option("tight_box", 1)
        for slot in (0, 1):
            assert same(_slot(slot, m, b, gs, crit), ref), (b["name"], "tight_box=1", slot)
        assert tight_batches() == before + 2, b["name"]
        api.set_option("tight_box", 0)
        assert same(_slot(0, m, b, gs, crit), ref), (b["name"], "tight_box=0 again")
        assert tight_batches() == before + 2
    finally:
        api.set_option("tight_box", 1)
    return ref


@pytest.mark.device_solve
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_slots_loose_and_tight(gpu, batches, kind):
    crit = api.ICPConvergenceCriteria(0.0, 0.0, 3)
    for k, b in enumerate(batches):
        m = api.Model(tris=b["tris"])                            # a buffer of its own: its first batch is loose, the list comes with the second
        _loose_then_tight(m, b, _scenes(k, b, kind)[0], crit)


@pytest.mark.device_solve
def test_slots_offsets_restart_at_every_sub_batch(gpu, batches):
    """sub_batch 32: the shuffled whole-frame, few-pixel and empty boxes of a batch land in different sub-batches, each packed from offset 0."""
    try:
        api.set_option("sub_batch", 32)
        for k in (0, 1):
            b = batches[k]
            assert len(b["poses"]) > 64
            _loose_then_tight(api.Model(tris=b["tris"]), b, _scenes(k, b, "proj")[0], api.ICPConvergenceCriteria(0.0, 0.0, 2))
    finally:
        api.set_option("sub_batch", 512)


# ---- a mixed batch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_mixed_batch_of_soup_and_shell(gpu, batches, models, solve):
    """Soup and shell hypotheses interleaved, a few of an empty third mesh among them: every record is the single-mesh call's, every size the oracle's."""
    a, s = batches[0], batches[1]
    assert a["name"] == "soup" and s["name"] == "shell" and np.array_equal(a["K"], s["K"]) and len(a["poses"]) == len(s["poses"])
    n = len(a["poses"])
    poses = np.empty((2 * n, 4, 4), np.float32)
    poses[0::2], poses[1::2] = a["poses"], s["poses"]
    R = np.empty((2 * n, H, W), np.int32)
    R[0::2], R[1::2] = a["R"], s["R"]
    idx = np.arange(2 * n) % 2
    empty = [7, 40, 101]
    idx[empty] = 2
    R[empty] = 0
    meshes = [models[0], models[1], np.zeros((0, 3, 3), np.float32)]
    proj, K = a["proj"], a["K"]
    drawn = drawn_count(R)
    for dtype in DTYPES:
        scene = _scene(a, dtype)
        got = api.score_poses_multi(meshes, idx, poses, W, H, proj, scene, TAU)
        want = np.zeros(2 * n, api.SCORE)
        for mi in (0, 1):
            sel = np.flatnonzero(idx == mi)
            want[sel] = api.score_poses(meshes[mi], poses[sel], W, H, proj, scene, TAU)
        assert got.tobytes() == want.tobytes()
        assert_scores_equal(got, score_ref(R, scene, TAU))
        assert np.array_equal(got["visible"], drawn)
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 3)
        for kind in ("proj", "nn"):
            gs = _scenes(0, a, kind)[0]
            res, sizes = api.refine_batch_multi(meshes, idx, poses, W, H, proj, K, gs, crit)
            assert np.array_equal(sizes, drawn), kind
            for mi in (0, 1):
                sel = np.flatnonzero(idx == mi)
                one, osz = api.refine_batch(meshes[mi], poses[sel], W, H, proj, K, gs, crit)
                assert np.array_equal(sizes[sel], osz) and res[sel].tobytes() == one.tobytes(), (kind, mi)
            assert (sizes[empty] == 0).all() and np.array_equal(res["T"][empty], np.tile(np.eye(4, dtype=np.float32).reshape(16), (3, 1)))
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------------------
def _level_counts(R, stride):
    """Per hypothesis the drawn pixels whose FRAME column and row are multiples of `stride`."""
    return drawn_count(R[:, ::stride, ::stride])


@pytest.mark.parametrize("solve", [api.SOLVE_HOST, api.SOLVE_DEVICE])
def test_pyramid(gpu, batches, models, solve):
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 3)
        levels = ((4, (0.0, 0.0, 3)), (1, (0.0, 0.0, 2)))
        ppb = api.get_option("points_per_block")
        for k, (b, m) in enumerate(zip(batches, models)):
            gs, osc = _scenes(k, b, "proj")
            want, wsizes = api.refine_batch(m, b["poses"], W, H, b["proj"], b["K"], gs, crit)
            res, lres, lsizes = api.refine_pyramid(m, b["poses"], W, H, b["proj"], b["K"], gs, [api.PyramidLevel(1, crit)], return_levels=True)
            assert np.array_equal(lsizes[0], wsizes) and np.array_equal(wsizes, _drawn(b)), b["name"]
            assert res.tobytes() == want.tobytes() and lres[0].tobytes() == want.tobytes(), b["name"]
            res, lres, lsizes = api.refine_pyramid(m, b["poses"], W, H, b["proj"], b["K"], gs, levels, return_levels=True)
            assert np.array_equal(lsizes[0], _level_counts(b["R"], 4)), b["name"]
            assert np.array_equal(lsizes[1], _level_counts(b["R"], 1)), b["name"]
            ores, olres, olsizes = _cached(("pyramid", k, ppb), lambda: pyramid_ref.refine_pyramid(b["tris"], b["poses"], W, H, b["proj"], b["K"], osc, levels, ppb))
            assert np.array_equal(lsizes, olsizes), b["name"]
            for got_l, want_l, sizes_l, what in ((lres[0], olres[0], lsizes[0], "level 0"), (lres[1], olres[1], lsizes[1], "level 1"), (res, ores, lsizes[1], "final")):
                worst = float(np.abs(got_l["T"].astype(np.float64) - want_l["T"].astype(np.float64)).max())
                print(f"{b['name']} {what}: max |T - T_ref| = {worst:.3g}")
                assert np.array_equal(got_l["fitness"], want_l["fitness"]), (b["name"], what)
                assert np.array_equal(inliers(got_l["fitness"], sizes_l), inliers(want_l["fitness"], sizes_l)), (b["name"], what)
                assert np.allclose(got_l["inlier_rmse"], want_l["inlier_rmse"], rtol=1e-6, atol=0), (b["name"], what)
                assert np.allclose(got_l["T"], want_l["T"], rtol=0, atol=TOL_T), (b["name"], what, worst)
    finally:
        api.set_option("solve", api.SOLVE_HOST)


# ---- two boxes at once: visible surface discrepancy over the union of a pair's boxes ---------------------------------------------------------
def _soup_and_shell(batches):
    a, s = batches[0], batches[1]
    assert a["name"] == "soup" and s["name"] == "shell" and np.array_equal(a["K"], s["K"]) and len(a["poses"]) == len(s["poses"])
    return a, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_k", [True, False])
def test_pose_vsd(gpu, batches, models, with_k, dtype):
    """Estimate i against hypothesis perm[i] of the same batch (box_stress.vsd_pairing), then every estimate against one truth whose box is the
    frame and against one that draws nothing: every record byte for byte vsd_ref's over the oracle's renders."""
    for k, (b, m) in enumerate(zip(batches, models)):
        scene, K, R = _scene(b, dtype), (b["K"] if with_k else None), b["R"]
        perm = vsd_pairing(len(R))
        got = api.pose_vsd(m, b["poses"], b["poses"][perm], W, H, b["proj"], scene, K, VSD_DELTA, SMALL_TAUS)
        assert_vsd_equal(got, vsd_reference(k, with_k))
        for t in one_truths(k):
            got = api.pose_vsd(m, b["poses"], b["poses"][t], W, H, b["proj"], scene, K, VSD_DELTA, SMALL_TAUS)
            assert_vsd_equal(got, _cached(("vsd one", k, t, with_k), lambda: vsd_ref(R, R[t], b["scene"], K, VSD_DELTA, SMALL_TAUS)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pose_vsd_mixed_batch_of_soup_and_shell(gpu, batches, models, dtype):
    """Soup and shell pairs interleaved: pair i is held to the renders of its own mesh."""
    a, s = _soup_and_shell(batches)
    perm = vsd_pairing(len(a["poses"]))
    est, gt = interleaved(a["poses"], s["poses"]), interleaved(a["poses"][perm], s["poses"][perm])
    r_est, r_gt = interleaved(a["R"], s["R"]), interleaved(a["R"][perm], s["R"][perm])
    idx = np.arange(len(est)) % 2
    for K in (a["K"], None):
        got = api.pose_vsd_multi(models[:2], idx, est, gt, W, H, a["proj"], _scene(a, dtype), K, VSD_DELTA, SMALL_TAUS)
        assert_vsd_equal(got, vsd_ref(r_est, r_gt, a["scene"], K, VSD_DELTA, SMALL_TAUS))


# ---- ... interpenetration over the intersection of two boxes, in LDS bands; the far plane ----------------------------------------------------
def _planes_of(m, poses, proj):
    near, far = api.render_span(m, poses, W, H, proj)
    return near.to_host().reshape(len(poses), H, W), far.to_host().reshape(len(poses), H, W)


def _assert_pairs(got, want, what):
    assert got.dtype == api.PAIR_SOLID and got.shape == want.shape, what
    for f in api.PAIR_SOLID.names:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (what, f, len(bad), bad[:5].tolist(), [(int(got[f][i, j]), int(want[f][i, j])) for i, j in bad[:5]])
    assert got.tobytes() == want.tobytes(), what
    check_pair_invariants(got)


def test_render_span_near_and_far_plane(gpu, batches, models):
    """Both planes of pr_render_span on every batch: the near plane is R (negative depths and all), the far plane solid_ref's maximum
    composite -- also where fragments lie behind the camera."""
    behind = 0
    for k, (b, m) in enumerate(zip(batches, models)):
        near, far = _planes_of(m, b["poses"], b["proj"])
        want_near, want_far = returned_planes(k)
        for got, want, plane in ((near, want_near, "near"), (far, want_far, "far")):
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (b["name"], plane, len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)], want[tuple(bad[:5].T)])
        assert np.array_equal(near, b["R"]), b["name"]
        behind += int((near < 0).any((1, 2)).sum())
    assert behind >= 4


@pytest.mark.parametrize("slack", SLACKS)
def test_pose_penetration(gpu, batches, models, slack):
    for k, (b, m) in enumerate(zip(batches, models)):
        _assert_pairs(api.pose_penetration(m, b["poses"], W, H, b["proj"], slack), pair_records(k, slack), (b["name"], slack))


def test_pose_penetration_mixed_batch_of_soup_and_shell(gpu, batches, models):
    a, s = _soup_and_shell(batches)
    poses = interleaved(a["poses"], s["poses"])
    idx = np.arange(len(poses)) % 2
    near, far = span_ref_multi([a["tris"], s["tris"]], idx, poses, a["proj"], W, H)
    assert np.array_equal(near[0::2], span_planes(0)[0]) and np.array_equal(far[1::2], span_planes(1)[1])
    for slack in SLACKS:
        _assert_pairs(api.pose_penetration_multi(models[:2], idx, poses, W, H, a["proj"], slack), pairs_ref(near, far, slack), ("mixed", slack))


# ---- ... the overlap matrix over the saved boxes of all P hypotheses -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("roi", [NONE] + ROIS)
def test_score_overlap(gpu, batches, models, roi, dtype):
    shared = 0
    for k, (b, m) in enumerate(zip(batches, models)):
        r, want_sc = _score_ref(k, b, roi)
        want_ov = _cached(("overlap", k, roi), lambda: overlap_ref(r, b["scene"], TAU, roi))
        sc, ov = api.score_overlap(m, b["poses"], W, H, b["proj"], _scene(b, dtype), TAU, roi=roi)
        _assert_overlap(sc, ov, want_sc, want_ov)
        assert sc.tobytes() == want_sc.tobytes(), b["name"]
        shared += int(np.count_nonzero(np.triu(want_ov, 1)))
    assert shared >= 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_overlap_mixed_batch_of_soup_and_shell(gpu, batches, models, dtype):
    a, s = _soup_and_shell(batches)
    poses, R = interleaved(a["poses"], s["poses"]), interleaved(a["R"], s["R"])
    idx = np.arange(len(poses)) % 2
    sc, ov = api.score_overlap_multi(models[:2], idx, poses, W, H, a["proj"], _scene(a, dtype), TAU)
    _assert_overlap(sc, ov, score_ref(R, a["scene"], TAU), _cached(("overlap mixed",), lambda: overlap_ref(R, a["scene"], TAU)))
    assert ov[0::2, 1::2].any()                                   # hypotheses of different meshes do share inliers


# ---- the contour fit: 4-neighbours across the box edge and the window edge -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tjr", [FIT_TJR, FIT_TJR_WIDE])
def test_contour_information(gpu, batches, models, tjr, dtype):
    """The nearest-edge map bit for bit; the integer fields of every record exactly and the 30 sums within contour_fit_ref.fit_bound of the
    reference over the oracle's renders -- on the offset meshes too, whose model centre lies 10^3 .. 10^7 mm from the origin (the centre
    enters the sums only through c = pose applied to it, which the offset poses bring back in front of the camera)."""
    tau, jump, radius = tjr
    worst = 0.0
    for k, (b, m) in enumerate(zip(batches, models)):
        scene = _scene(b, dtype)
        nd = api.scene_edge_nearest(scene, W, H, jump, radius)
        assert np.array_equal(nd.to_host().reshape(H, W), nearest_map(k, jump, radius)), b["name"]
        cs, rho = model_centres(k)
        for roi in (NONE, ROIS[1]):
            sc, fit, info = api.contour_information(m, b["poses"], W, H, b["proj"], b["K"], scene, tau, jump, nd, roi=roi if roi != NONE else None)
            worst = max(worst, assert_records(fit, info, fit_reference(k, tjr, roi), cs, rho, (b["name"], tjr, roi)))
            assert_scores_equal(sc, _cached(("score", k, roi, tau), lambda: score_ref(b["R"] if roi == NONE else roi_renders(k, roi), b["scene"], tau, roi)))
    print(tjr, np.dtype(dtype).name, "largest error / bound", worst)


def test_contour_information_mixed_batch_of_soup_and_shell(gpu, batches, models):
    a, s = _soup_and_shell(batches)
    poses = interleaved(a["poses"], s["poses"])
    idx = np.arange(len(poses)) % 2
    tau, jump, radius = FIT_TJR_WIDE
    nd = api.scene_edge_nearest(a["scene"], W, H, jump, radius)
    N = nearest_map(0, jump, radius)
    _, fit, info = api.contour_information_multi(models[:2], idx, poses, W, H, a["proj"], a["K"], a["scene"], tau, jump, nd)
    for mi, b in enumerate((a, s)):
        cs, rho = model_centres(mi)
        refs = fit_reference(0, FIT_TJR_WIDE) if mi == 0 else _cached(("fit shell on soup",), lambda: CF.fit_records(b["R"], a["scene"], N, tau, jump, a["K"], cs, rho))
        assert_records(fit[mi::2], info[mi::2], refs, cs, rho, ("mixed", b["name"]))


# ---- the fused information pass: its clouds are what render + emit leave in the boxes ---------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pose_information_cloud_sizes(gpu, batches, models, dtype):
    for k, (b, m) in enumerate(zip(batches, models)):
        info, _, sizes = api.pose_information(m, b["poses"], W, H, b["proj"], b["K"], _scenes(k, b, "proj", dtype)[0], want_eig=False)
        assert np.array_equal(sizes, _drawn(b)), (b["name"], np.flatnonzero(sizes != _drawn(b))[:10])
        assert np.array_equal(info["n_points"], _drawn(b)), b["name"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [0, 1], ids=["soup", "shell"])
def test_pose_information_records(gpu, batches, models, k, dtype):
    """Every hypothesis that draws a pixel: the record against info_ref.record on the oracle's cloud of the oracle's render (fragments behind
    the camera are no points), the correspondences the library's own, within info_ref.sum_bound."""
    b, m = batches[k], models[k]
    gs = _scenes(k, b, "proj", dtype)[0]
    info, _, sizes = api.pose_information(m, b["poses"], W, H, b["proj"], b["K"], gs, want_eig=False)
    cs, rho = model_centres(k)
    assert np.array_equal(info["c"], cs) and (info["rho"] == np.float32(rho)).all()
    kit = Kit(gs, packed=True)
    worst, held = 0.0, 0
    for i in np.flatnonzero(_drawn(b) >= 1):
        cloud = O.depth2cloud(np.maximum(b["R"][i], 0), b["K"])
        assert len(cloud) == sizes[i], (b["name"], i)
        worst = max(worst, assert_record(info[i], info_ref.record(cloud, kit.associate(cloud), None, cs[i], rho), (b["name"], i, b["families"][i])))
        held += 1
    print(b["name"], np.dtype(dtype).name, held, "records, largest error / bound", worst)
    assert held >= 40 and info["n_valid"].sum() > 10000
