"""GPU tests (-m gpu) of the contour check: pr_scene_edge_distance_dev and pr_score_contours held to the numpy restatement of the header's
definitions (tests/contour_ref.py) over the oracle's renders -- every integer field bit-exact, int32 and uint16 scenes, with and without ROI."""
import threading

import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import W, H, raw_h2d
from contour_ref import (NO_EDGE, assert_contours_equal, contour_ref, edge_distance_ref, edges, jump_only, structured_scene)
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import assert_scores_equal, launch_split_case, score_ref

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
# the windows of test_verify_gpu.py; the last one cuts the object
ROIS_INSIDE = [(200, 150, 200, 180), (0, 0, W, H), (0, 100, 330, 200), (100, 0, 300, 240), (W - 320, 100, 320, 200),
               (100, H - 240, 300, 240), (300, 230, 60, 40)]
ZERO_FIELDS = ("contour", "hit", "occluded", "miss", "dist_sum")


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)                                  # configs[1] sampler


@pytest.fixture(scope="module")
def scene(scenario):
    return structured_scene(scenario["depth"][1])


@pytest.fixture(scope="module")
def renders(scenario, hyps):
    return O.render(scenario["tris"], hyps, W, H, scenario["proj"])


def _as(scene, dtype):
    return np.ascontiguousarray(scene.astype(dtype))


def _dist_host(dv, h, w):
    return dv.to_host().reshape(h, w)


# ---- the scene's edge distance ---------------------------------------------------------------------------------------------------------
def _blocky_frame(rng, h, w):
    """Random surfaces in rectangles over holes: edges of every orientation, at the frame border too."""
    d = np.zeros((h, w), np.int64)
    for _ in range(max(4, h * w // 400)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        d[y0:y0 + int(rng.integers(1, 30)), x0:x0 + int(rng.integers(1, 30))] = int(rng.integers(0, 6)) * 7 + 300
    return d


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("radius", [0, 1, 3, 32])
def test_edge_distance_structured_scene(gpu, scene, dtype, radius):
    s = _as(scene, dtype)
    sd = api.DeviceVector.from_host(s.reshape(-1))
    for jump in (0, 10, 60000):
        got = _dist_host(api.scene_edge_distance(sd, W, H, jump, radius), H, W)
        want = edge_distance_ref(s, jump, radius)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (jump, np.argwhere(got != want)[:5])
        assert (got == 0).sum() == edges(s, jump).sum() > 0
        assert (got == NO_EDGE).any() and got[got != NO_EDGE].max() == radius


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2), (37, 65), (50, 200), (77, 333), (64, 128), (5, 1000)])
def test_edge_distance_frame_shapes(gpu, shape):
    """Frames of width 1 and of height 1, widths that are no multiple of 64 (and some that are), an all-empty frame of every shape."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    d = _blocky_frame(rng, h, w)
    for dtype in (np.int32, np.uint16):
        for frame in (d, np.zeros_like(d), np.full_like(d, 500)):
            s = _as(frame, dtype)
            for jump, radius in ((0, 0), (6, 1), (6, 3), (13, 32), (100, 32)):
                got = _dist_host(api.scene_edge_distance(s, w, h, jump, radius), h, w)
                assert np.array_equal(got, edge_distance_ref(s, jump, radius)), (shape, dtype, jump, radius)
            if not frame.any() or frame.all():
                assert (got == NO_EDGE).all()                     # no surface at all, or one flat surface up to the border: no edge


def test_edge_distance_int32_extremes(gpu):
    """Scene values at both ends of int32: <= 0 is empty, and d_n - d does not overflow."""
    rng = np.random.default_rng(8)
    h, w = 96, 150
    vals = np.array([INT32_MAX, INT32_MAX - 1, INT32_MAX - 1000, 1, 2, 300, 0, -1, -INT32_MAX - 1], np.int64)
    ext = np.repeat(np.repeat(rng.choice(vals, size=(h // 3, w // 3)), 3, 0), 3, 1).astype(np.int32)
    seen = set()
    for jump in (0, 1, 998, 999, 1000, INT32_MAX - 3, INT32_MAX - 2, INT32_MAX):
        got = _dist_host(api.scene_edge_distance(ext, w, h, jump, 2), h, w)
        assert np.array_equal(got, edge_distance_ref(ext, jump, 2)), jump
        seen.add(int((got == 0).sum()))
    assert len(seen) >= 4                                         # the jump matters up to the largest difference two int32 values have


def test_edge_distance_argument_errors(gpu, scene):
    lib = _lib.load()
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    out = api.DeviceVector(W * H, np.uint8)
    canary = np.full(W * H, 77, np.uint8)
    raw_h2d(out.data(), canary)
    for args in ((None, 1, W, H, 10, 3, out.data()), (sd.data(), 1, W, H, 10, 3, None), (sd.data(), 1, 0, H, 10, 3, out.data()),
                 (sd.data(), 1, W, 0, 10, 3, out.data()), (sd.data(), 1, W, H, -1, 3, out.data()), (sd.data(), 1, W, H, 10, 33, out.data()),
                 (sd.data(), 1, 8193, 4, 10, 3, out.data())):
        assert lib.pr_scene_edge_distance_dev(*args) == _lib.PR_ERR_INVALID, args
    assert np.array_equal(out.to_host(), canary)                  # nothing written
    with pytest.raises(api.PoseRefineError) as e:
        api.scene_edge_distance(sd, W, H, 10, api.CONTOUR_MAX_RADIUS + 1)
    assert e.value.code == _lib.PR_ERR_INVALID
    assert lib.pr_scene_edge_distance_dev(sd.data(), 1, W, H, 10, api.CONTOUR_MAX_RADIUS, out.data()) == _lib.PR_OK


# ---- contour records ---------------------------------------------------------------------------------------------------------------------
_REF_CACHE = {}


def _want(renders, scene, tau, jump, radius):
    """The reference for the 256 hypotheses (the same for both scene types: the scene's values fit uint16)."""
    key = (tau, jump, radius)
    if key not in _REF_CACHE:
        D = edge_distance_ref(scene, jump, radius)
        _REF_CACHE[key] = (D, contour_ref(renders, scene, tau, jump, D))
    return _REF_CACHE[key]


def _jump_only_total(renders, jump):
    if ("jump_only", jump) not in _REF_CACHE:
        _REF_CACHE[("jump_only", jump)] = sum(int(jump_only(renders[i:i + 32], jump).sum()) for i in range(0, len(renders), 32))
    return _REF_CACHE[("jump_only", jump)]


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tjr", [(5, 10, 4), (5, 4, 2), (5, 30, 2), (0, 10, 0), (20, 30, 4)])
def test_parity_256_hypotheses(gpu, model, scenario, hyps, scene, renders, tjr, dtype):
    tau, jump, radius = tjr
    s = _as(scene, dtype)
    sd = api.DeviceVector.from_host(s.reshape(-1))
    ed = api.scene_edge_distance(sd, W, H, jump, radius)
    D, want = _want(renders, scene, tau, jump, radius)
    assert np.array_equal(_dist_host(ed, H, W), D)
    scores, got = api.score_contours(model, hyps, W, H, scenario["proj"], sd, tau, jump, ed)
    assert_contours_equal(got, want)
    assert scores.tobytes() == api.score_poses(model, hyps, W, H, scenario["proj"], sd, tau).tobytes()
    for f in ("contour", "hit", "occluded", "miss"):              # every class occurs, or the test proves little
        assert got[f].sum() > 0, f
    if radius > 0:                                                # ... and with a radius, for every one of the 256 hypotheses
        for f in ("contour", "hit", "occluded", "miss", "dist_sum"):
            assert (want[f] > 0).all() and (got[f] > 0).all(), f
    else:
        assert got["dist_sum"].sum() == 0                         # radius 0: a hit lies on a scene edge
    assert _jump_only_total(renders, jump) > 1000                 # contours inside the silhouette, which only the jump rule finds


def test_overlap_from_the_same_render(gpu, model, scenario, hyps, scene):
    for dt in (np.int32, np.uint16):
        sd = api.DeviceVector.from_host(_as(scene, dt).reshape(-1))
        ed = api.scene_edge_distance(sd, W, H, 10, 3)
        scores, con, ov = api.score_contours(model, hyps, W, H, scenario["proj"], sd, 5, 10, ed, want_overlap=True)
        s2, ov2 = api.score_overlap(model, hyps, W, H, scenario["proj"], sd, 5)
        assert scores.tobytes() == s2.tobytes() and ov.tobytes() == ov2.tobytes() and ov.shape == (256, 256)
        s3, con3 = api.score_contours(model, hyps, W, H, scenario["proj"], sd, 5, 10, ed)
        assert s3.tobytes() == scores.tobytes() and con3.tobytes() == con.tobytes()
        assert np.array_equal(np.diag(ov), scores["inlier"]) and con["contour"].min() > 0


@pytest.mark.parametrize("roi", ROIS_INSIDE)
def test_roi_parity(gpu, model, scenario, hyps, scene, roi):
    poses = hyps[:64]
    D = edge_distance_ref(scene, 10, 3)
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"], roi)
    want = contour_ref(r, scene, 10, 10, D, roi)
    for dt in (np.int32, np.uint16):
        s = _as(scene, dt)
        ed = api.scene_edge_distance(s, W, H, 10, 3)
        scores, got = api.score_contours(model, poses, W, H, scenario["proj"], s, 10, 10, ed, roi=roi)
        assert_contours_equal(got, want)
        assert_scores_equal(scores, score_ref(r, s, 10, roi))
    if roi == (300, 230, 60, 40):                                 # a window that cuts the object: the cut itself is no contour
        full = api.score_contours(model, poses, W, H, scenario["proj"], scene, 10, 10, ed)[1]
        assert (got["contour"] > 0).any() and (got["contour"] < full["contour"]).all()
        padded = sum(int(edges(np.pad(img, 1), 10).sum()) for img in r)
        assert padded > int(got["contour"].sum())


def test_hypothesis_across_the_frame_border(gpu, model, scenario, scene):
    """The object pushed over the left, right, top and bottom border of the frame: it is cut there, and the cut is no contour."""
    base = scenario["poses"][1]
    poses = np.stack([base.copy() for _ in range(5)])
    poses[0, 0, 3] -= 175.0
    poses[1, 0, 3] += 170.0
    poses[2, 1, 3] -= 135.0
    poses[3, 1, 3] += 125.0
    poses[4, 0, 3] -= 185.0
    poses[4, 1, 3] += 110.0                                       # a corner
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    borders = [r[0][:, 0], r[1][:, W - 1], r[2][0, :], r[3][H - 1, :], r[4][:, 0], r[4][H - 1, :]]
    assert all((b > 0).sum() > 5 for b in borders), [(b > 0).sum() for b in borders]
    D = edge_distance_ref(scene, 10, 3)
    want = contour_ref(r, scene, 5, 10, D)
    for dt in (np.int32, np.uint16):
        s = _as(scene, dt)
        got = api.score_contours(model, poses, W, H, scenario["proj"], s, 5, 10, api.scene_edge_distance(s, W, H, 10, 3))[1]
        assert_contours_equal(got, want)
    for i in range(5):                                            # with the border counted as empty, the cut would be contour
        assert int(edges(np.pad(r[i], 1), 10).sum()) > int(want["contour"][i]) > 0


def test_self_consistency_and_shift(gpu, model, scenario):
    """The scene pose against its own render, and hits falling as the pose is pushed sideways (radius 3, jump 10, tau 5)."""
    d1 = scenario["depth"][1]
    for dt in (np.int32, np.uint16):
        s = _as(d1, dt)
        ed = api.scene_edge_distance(s, W, H, 10, 3)
        assert (_dist_host(ed, H, W) == 0).sum() == 823
        poses = np.stack([scenario["poses"][1].copy() for _ in range(5)])
        poses[1:, 0, 3] += np.array([2, 5, 10, 20], np.float32)
        scores, c = api.score_contours(model, poses, W, H, scenario["proj"], s, 5, 10, ed)
        assert (c["contour"][0], c["hit"][0], c["occluded"][0], c["miss"][0], c["dist_sum"][0]) == (823, 823, 0, 0, 0)
        assert c["hit"][1:].tolist() == [672, 320, 196, 142] and c["miss"][1:].tolist() == [21, 273, 368, 446]
        assert c["hit"][2] >= c["hit"][3] >= c["hit"][4]          # past the radius, hits do not come back
        assert scores["inlier"][0] == np.count_nonzero(d1)
        frac = api.contour_fraction(c)
        assert frac[0] == 1.0 and (np.diff(frac) < 0).all()
        assert api.filter_by_contour(np.arange(5), c, 0.6).tolist() == [0, 1]


def test_edge_cases(gpu, model, scenario, hyps, scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    ed = api.scene_edge_distance(sd, W, H, 10, 3)
    # no hypotheses: PR_OK, nothing written (null pointers allowed)
    assert lib.pr_score_contours(None, 0, None, 0, W, H, pj.ctypes.data, _lib.Roi(0, 0, 0, 0), None, 1, 5, 10, None, None, None, None) == _lib.PR_OK
    sc, con = api.score_contours(model, np.zeros((0, 4, 4), np.float32), W, H, pj, sd, 5, 10, ed)
    assert len(sc) == 0 and len(con) == 0
    sc, con = api.score_contours_multi([model], np.zeros(0, np.int64), np.zeros((0, 4, 4), np.float32), W, H, pj, sd, 5, 10, ed)
    assert len(sc) == 0 and len(con) == 0
    # behind the camera / off-screen: all zeros
    odd = np.stack([hyps[1].copy(), hyps[2].copy(), hyps[3].copy()])
    odd[0, 2, 3] = -300.0
    odd[1, 0, 3] = 1.0e6
    con = api.score_contours(model, odd, W, H, pj, sd, 5, 10, ed)[1]
    for f in ZERO_FIELDS:
        assert con[f][0] == 0 and con[f][1] == 0, f
    assert con["contour"][2] > 0
    # an empty mesh renders nothing
    empty = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    con = api.score_contours(empty, hyps[:5], W, H, pj, sd, 5, 10, ed)[1]
    assert all((con[f] == 0).all() for f in ZERO_FIELDS)
    # extreme int32 scene values: occluded needs r - s in 64 bits
    poses = hyps[:16]
    r = O.render(scenario["tris"], poses, W, H, pj)
    rng = np.random.default_rng(5)
    ext = rng.choice(np.array([INT32_MAX, INT32_MAX - 1, -1, -INT32_MAX - 1, 0, 300, 1], np.int64), size=(H, W)).astype(np.int32)
    D = edge_distance_ref(scene, 10, 3)
    for tau in (0, 1000, INT32_MAX):
        got = api.score_contours(model, poses, W, H, pj, ext, tau, 10, ed)[1]
        assert_contours_equal(got, contour_ref(r, ext, tau, 10, D))
    for jump in (0, INT32_MAX):                                   # a jump no render can reach: only the silhouette is contour
        got = api.score_contours(model, poses, W, H, pj, sd, 5, jump, ed)[1]
        assert_contours_equal(got, contour_ref(r, scene, 5, jump, D))
    assert jump_only(r, INT32_MAX).sum() == 0 and jump_only(r, 0).sum() > 0


def test_argument_errors(gpu, model, scenario, hyps, scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    ed = api.scene_edge_distance(sd, W, H, 10, 3)
    poses = np.ascontiguousarray(hyps[:16], np.float32)
    td = model.device_tris()
    sc = np.zeros(16, api.SCORE)
    con = np.zeros(16, api.CONTOUR)
    no_roi = _lib.Roi(0, 0, 0, 0)

    def call(tau=5, jump=10, scene_p=sd.data(), ed_p=ed.data(), sc_p=sc.ctypes.data, con_p=con.ctypes.data, roi=no_roi, n=16, ov=None):
        return lib.pr_score_contours(td.data(), td.size() // 9, poses.ctypes.data, n, W, H, pj.ctypes.data, roi, scene_p, 1, tau, jump, ed_p, sc_p, con_p, ov)

    for kw in (dict(tau=-1), dict(jump=-1), dict(ed_p=None), dict(con_p=None), dict(sc_p=None), dict(scene_p=None), dict(roi=_lib.Roi(600, 0, 100, 100)),
               dict(jump=-1, n=0)):
        assert call(**kw) == _lib.PR_ERR_INVALID, kw
    assert (sc["visible"] == 0).all() and all((con[f] == 0).all() for f in ZERO_FIELDS)      # nothing written
    table = (_lib.MeshRef * 1)(_lib.MeshRef(td.data(), td.size() // 9))
    idx = np.zeros(16, np.uint32)
    for jump, ed_p, con_p in ((-1, ed.data(), con.ctypes.data), (10, None, con.ctypes.data), (10, ed.data(), None)):
        assert lib.pr_score_contours_multi(table, 1, idx.ctypes.data, poses.ctypes.data, 16, W, H, pj.ctypes.data, no_roi, sd.data(), 1, 5, jump, ed_p,
                                           sc.ctypes.data, con_p, None) == _lib.PR_ERR_INVALID
    assert (sc["visible"] == 0).all() and all((con[f] == 0).all() for f in ZERO_FIELDS)
    assert call() == _lib.PR_OK and (con["contour"] > 0).all()
    with pytest.raises(api.PoseRefineError) as e:
        api.score_contours(model, hyps[:4], W, H, pj, sd, 5, -3, ed)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_score_contours: jump_mm" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:                 # the message names the entry point that was called
        api.score_contours_multi([model], np.zeros(4, np.int64), hyps[:4], W, H, pj, sd, -1, 10, ed)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_score_contours_multi: tau_mm" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:                 # the overlap matrix keeps its limit
        api.score_contours(model, np.tile(hyps[:1], (api.OVERLAP_MAX_POSES + 1, 1, 1)), W, H, pj, sd, 5, 10, ed, want_overlap=True)
    assert e.value.code == _lib.PR_ERR_INVALID
    with pytest.raises(ValueError):
        api.score_contours(model, hyps[:4], W, H, pj, sd, 5, 10, api.DeviceVector(W * H - 1, np.uint8))


def test_multi_mesh_matches_single_mesh_calls(gpu, scenario, hyps, scene):
    """8 meshes x 32 hypotheses in shuffled order: every record is what one single-mesh call per mesh gives."""
    t = scenario["tris"]
    meshes = [np.ascontiguousarray(t * np.float32(0.65 + 0.07 * k)) for k in range(7)] + [np.zeros((0, 3, 3), np.float32)]
    idx = np.random.default_rng(3).permutation(np.repeat(np.arange(8), 32))
    for dt in (np.int32, np.uint16):
        sd = api.DeviceVector.from_host(_as(scene, dt).reshape(-1))
        ed = api.scene_edge_distance(sd, W, H, 10, 3)
        sc, con, ov = api.score_contours_multi(meshes, idx, hyps, W, H, scenario["proj"], sd, 5, 10, ed, want_overlap=True)
        want_sc, want_con = np.zeros(256, api.SCORE), np.zeros(256, api.CONTOUR)
        for m in range(8):
            sel = np.flatnonzero(idx == m)
            assert len(sel) == 32
            want_sc[sel], want_con[sel] = api.score_contours(meshes[m], hyps[sel], W, H, scenario["proj"], sd, 5, 10, ed)
        assert sc.tobytes() == want_sc.tobytes() and con.tobytes() == want_con.tobytes()
        s2, ov2 = api.score_overlap_multi(meshes, idx, hyps, W, H, scenario["proj"], sd, 5)
        assert s2.tobytes() == sc.tobytes() and ov2.tobytes() == ov.tobytes()
        sc3, con3 = api.score_contours_multi(meshes, idx, hyps, W, H, scenario["proj"], sd, 5, 10, ed)
        assert sc3.tobytes() == sc.tobytes() and con3.tobytes() == con.tobytes()
        assert (con["contour"][idx == 7] == 0).all() and (con["contour"][idx != 7] > 0).all()
        assert len(set(con["contour"][idx != 7].tolist())) > 50


def test_scene_and_distance_are_read_on_every_call(gpu, model, scenario, hyps, scene, renders):
    poses, r = hyps[:64], renders[:64]
    for dt in (np.int32, np.uint16):
        s1 = _as(scene, dt)
        s2 = _as(scenario["depth"][1], dt)
        D1, D2 = edge_distance_ref(s1, 10, 3), edge_distance_ref(s2, 10, 3)
        sd = api.DeviceVector.from_host(s1.reshape(-1))
        ed = api.scene_edge_distance(sd, W, H, 10, 3)
        assert_contours_equal(api.score_contours(model, poses, W, H, scenario["proj"], sd, 5, 10, ed)[1], contour_ref(r, s1, 5, 10, D1))
        raw_h2d(ed.data(), D2)                                    # the distance image overwritten behind the library's back
        assert_contours_equal(api.score_contours(model, poses, W, H, scenario["proj"], sd, 5, 10, ed)[1], contour_ref(r, s1, 5, 10, D2))
        raw_h2d(sd.data(), s2)                                    # ... and the scene
        assert_contours_equal(api.score_contours(model, poses, W, H, scenario["proj"], sd, 5, 10, ed)[1], contour_ref(r, s2, 5, 10, D2))
        D3 = np.ascontiguousarray((np.arange(W * H, dtype=np.int64) % 255).astype(np.uint8).reshape(H, W))     # any byte below 255 is a distance
        raw_h2d(ed.data(), D3)
        got = api.score_contours(model, poses, W, H, scenario["proj"], sd, 5, 10, ed)[1]
        assert_contours_equal(got, contour_ref(r, s2, 5, 10, D3))
        assert got["dist_sum"].max() > 254 * 3
        assert np.array_equal(_dist_host(api.scene_edge_distance(sd, W, H, 10, 3), H, W), D2)                   # the scene as it is now


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_contours_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, scene, solve):
    """A synchronous contour score (and an edge distance) while a batch is pending on a slot of the same context: both give what they give alone."""
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
        alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        ed0 = api.scene_edge_distance(scene, W, H, 10, 3)
        alone = api.score_contours(model, hyps[::-1], W, H, scenario["proj"], scene, 5, 10, ed0)
        api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        ed1 = api.scene_edge_distance(scene, W, H, 10, 3)
        mid = api.score_contours(model, hyps[::-1], W, H, scenario["proj"], scene, 5, 10, ed1)
        res, sizes = api.refine_wait(0)
    finally:
        api.set_option("solve", before)
    assert np.array_equal(ed0.to_host(), ed1.to_host())
    assert mid[0].tobytes() == alone[0].tobytes() and mid[1].tobytes() == alone[1].tobytes()
    assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()


def test_private_context_gives_the_same_records(gpu, model, scenario, hyps, scene):
    ed = api.scene_edge_distance(scene, W, H, 10, 3)
    shared = api.score_contours(model, hyps, W, H, scenario["proj"], scene, 5, 10, ed)
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                mine = api.scene_edge_distance(scene, W, H, 10, 3)
                box["ed"] = mine.to_host()
                box["out"] = api.score_contours(model, hyps, W, H, scenario["proj"], scene, 5, 10, mine)
                box["shared_ed"] = api.score_contours(model, hyps, W, H, scenario["proj"], scene, 5, 10, ed)
                mine.free()
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert np.array_equal(box["ed"], ed.to_host())
    for k in ("out", "shared_ed"):
        assert box[k][0].tobytes() == shared[0].tobytes() and box[k][1].tobytes() == shared[1].tobytes()


def test_chunked_batch_matches_small_batches(gpu, model):
    """The 8192 x 2048 frame of test_verify_gpu.py (2^24 pixels): a chunk of the depth workspace holds 64 hypotheses, so 150 span three chunks."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    poses = synth.hypotheses(150, seed=9)
    scene = api.render_host(model, synth.scene_pose()[None], Wb, Hb, proj)[0]
    rng = np.random.default_rng(2)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    ed = api.scene_edge_distance(sd, Wb, Hb, 10, 2)
    whole = api.score_contours(model, poses, Wb, Hb, proj, sd, 4, 10, ed)
    parts = [api.score_contours(model, poses[i:i + 40], Wb, Hb, proj, sd, 4, 10, ed) for i in range(0, 150, 40)]
    assert_scores_equal(whole[0], np.concatenate([p[0] for p in parts]))
    assert_contours_equal(whole[1], np.concatenate([p[1] for p in parts]))
    assert whole[0].tobytes() == api.score_poses(model, poses, Wb, Hb, proj, sd, 4).tobytes()
    assert (whole[1]["contour"] > 0).all() and whole[1]["hit"].sum() > 0
    rows = slice(Hb // 2 - 150, Hb // 2 + 150)                    # the distance image of the large frame, where the object is
    got = _dist_host(ed, Hb, Wb)
    want = edge_distance_ref(scene[Hb // 2 - 160:Hb // 2 + 160], 10, 2)[10:-10]
    assert np.array_equal(got[rows], want) and (want == 0).sum() > 1000


def test_batch_of_two_box_launches(gpu):
    """32768 + 5 hypotheses in one depth chunk: the launches over their boxes are split in two (grid.y is limited).  Every score and contour
    record is the reference's for its pose, the ones behind the split included; int32 scene, no overlap matrix.  Behind the split every
    hypothesis takes the next pose (seam_cases.seam_index), so hypothesis 32768 + j never expects hypothesis j's records."""
    c = launch_split_case()
    idx = seam_index(c["P"], 8)
    poses = c["poses"][idx]
    ed = api.scene_edge_distance(c["scene"], c["W"], c["H"], c["jump"], c["radius"])
    assert np.array_equal(_dist_host(ed, c["H"], c["W"]), c["dist"])
    scores, got = api.score_contours(c["tris"], poses, c["W"], c["H"], c["proj"], c["scene"], c["tau"], c["jump"], ed)
    assert_seam_visible(c["contours"], idx)
    assert_records_take(got, c["contours"], idx)
    assert_records_take(scores, c["scores"], idx)
