"""GPU tests (-m gpu) of contour alignment: pr_scene_edge_nearest_dev bit-equal to the reference map, pr_contour_information held to
tests/contour_fit_ref.py over the oracle's renders -- the integer records byte for byte, every float64 sum within (2 used + 16) * 2^-52 * sum |term|
of math.fsum, which is pr_pose_info's bound with two terms per used pixel -- and api.refine_contours on the plate-on-wall case of the host test."""
import threading

import numpy as np
import pytest

import contour_fit_ref as CF
import info_ref as I
import oracle_lib as O
from contour_ref import NO_EDGE, edge_distance_ref, structured_scene
from gpu_common import H, W, raw_h2d
from pose_refine_amd import _lib, api, synth
from test_contour_fit_host import assert_plate_conditions
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import launch_split_case

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INT32_MAX = 2**31 - 1
TJR = [(5, 10, 4), (0, 10, 0), (20, 30, 32)]
ROIS = [(200, 150, 200, 180), (0, 100, 330, 200), (300, 230, 60, 40)]       # inside, at the frame's left border, cutting the object


def _as(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


# ---- the nearest map ---------------------------------------------------------------------------------------------------------------------------
def _blocky_frame(rng, h, w):
    d = np.zeros((h, w), np.int64)
    for _ in range(max(4, h * w // 400)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        d[y0:y0 + int(rng.integers(1, 30)), x0:x0 + int(rng.integers(1, 30))] = int(rng.integers(0, 6)) * 7 + 300
    return d


def _nearest_host(dv, h, w):
    return dv.to_host().reshape(h, w)


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2), (37, 65), (77, 333), (64, 128), (5, 1000)])
def test_nearest_frame_shapes(gpu, shape):
    h, w = shape
    d = _blocky_frame(np.random.default_rng(h * 1000 + w), h, w)
    for dtype in (np.int32, np.uint16):
        for frame in (d, np.zeros_like(d), np.full_like(d, 500)):
            s = _as(frame, dtype)
            for jump, radius in ((0, 0), (6, 1), (6, 3), (13, 32)):
                got = _nearest_host(api.scene_edge_nearest(s, w, h, jump, radius), h, w)
                assert got.dtype == np.uint32 and np.array_equal(got, CF.nearest_ref(s, jump, radius)), (shape, dtype, jump, radius)
                D = api.scene_edge_distance(s, w, h, jump, radius).to_host().reshape(h, w)
                assert np.array_equal(got != CF.NONE, D != NO_EDGE)
            if frame is not d:                                   # no surface at all, or one flat surface up to the border: no edge
                assert (got == CF.NONE).all()


def test_nearest_int32_extremes_and_arguments(gpu):
    rng = np.random.default_rng(8)
    h, w = 96, 150
    vals = np.array([INT32_MAX, INT32_MAX - 1, INT32_MAX - 1000, 1, 2, 300, 0, -1, -INT32_MAX - 1], np.int64)
    ext = np.repeat(np.repeat(rng.choice(vals, size=(h // 3, w // 3)), 3, 0), 3, 1).astype(np.int32)
    for jump in (0, 999, 1000, INT32_MAX - 2, INT32_MAX):
        for radius in (0, 1, 3, 32):
            assert np.array_equal(_nearest_host(api.scene_edge_nearest(ext, w, h, jump, radius), h, w), CF.nearest_ref(ext, jump, radius)), (jump, radius)
    lib = _lib.load()
    sd, out = api.DeviceVector.from_host(ext.reshape(-1)), api.DeviceVector(w * h, np.uint32)
    canary = np.full(w * h, 77, np.uint32)
    raw_h2d(out.data(), canary)
    for args in ((None, 1, w, h, 10, 3, out.data()), (sd.data(), 1, w, h, 10, 3, None), (sd.data(), 1, 0, h, 10, 3, out.data()), (sd.data(), 1, w, 0, 10, 3, out.data()),
                 (sd.data(), 1, w, h, -1, 3, out.data()), (sd.data(), 1, w, h, 10, 33, out.data()), (sd.data(), 1, 8193, 4, 10, 3, out.data())):
        assert lib.pr_scene_edge_nearest_dev(*args) == _lib.PR_ERR_INVALID, args
    assert np.array_equal(out.to_host(), canary)                    # nothing written


# ---- the records -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)[:32]


@pytest.fixture(scope="module")
def scene(scenario):
    return structured_scene(scenario["depth"][1])


@pytest.fixture(scope="module")
def renders(scenario, hyps):
    return O.render(scenario["tris"], hyps, W, H, scenario["proj"])


@pytest.fixture(scope="module")
def centre(model):
    return api._model_center_radius(model, None, None)


_NEAREST = {}


def _nearest(scene, jump, radius):
    if (jump, radius) not in _NEAREST:
        _NEAREST[(jump, radius)] = CF.nearest_ref(scene, jump, radius)
    return _NEAREST[(jump, radius)]


def assert_records(fit, info, refs, cs, rho, what):
    """fit: CONTOUR_FIT[P], info: POSE_INFO[P] of the device; refs: the reference records.  Returns the largest error / bound."""
    worst = 0.0
    for i, ref in enumerate(refs):
        for f in CF.FIT_FIELDS:
            assert int(fit[i][f]) == ref[f], (what, i, f, int(fit[i][f]), ref[f])
        assert (fit[i]["reserved"] == 0).all() and int(fit[i]["contour"]) == int(fit[i]["used"]) + int(fit[i]["occluded"]) + int(fit[i]["miss"])
        o = info[i]
        assert (int(o["n_points"]), int(o["n_valid"]), int(o["n_zero_weight"]), int(o["reserved"])) == (ref["contour"], ref["used"], 0, 0), (what, i)
        assert np.array_equal(o["c"], cs[i]) and o["rho"] == F32(rho), (what, i)
        got = I.flat_sums(o)
        err, bound = np.abs(got - ref["sums"]), CF.fit_bound(ref["used"], ref["abs"])
        assert (err <= bound).all(), (what, i, "columns", np.flatnonzero(err > bound), err[err > bound], bound[err > bound])
        assert o["sum_w"] == 2.0 * ref["used"] and o["sum_wr2"] == o["sum_r2"], (what, i)
        if ref["used"] == 0:
            assert not got.any(), (what, i)
        worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
    return worst


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("tjr", TJR)
def test_parity_32_hypotheses(gpu, model, scenario, hyps, scene, renders, centre, tjr, dtype):
    tau, jump, radius = tjr
    cm, rho = centre
    s = _as(scene, dtype)
    sd = api.DeviceVector.from_host(s.reshape(-1))
    nd = api.scene_edge_nearest(sd, W, H, jump, radius)
    N = _nearest(scene, jump, radius)
    assert np.array_equal(_nearest_host(nd, H, W), N)
    scores, fit, info = api.contour_information(model, hyps, W, H, scenario["proj"], scenario["K"], sd, tau, jump, nd)
    cs = CF.centers(hyps, cm)
    refs = CF.fit_records(renders, scene, N, tau, jump, scenario["K"], cs, rho)
    worst = assert_records(fit, info, refs, cs, rho, (tjr, dtype))
    print(tjr, dtype.__name__, "largest error / bound", worst, "used", fit["used"].min(), "..", fit["used"].max())
    assert scores.tobytes() == api.score_poses(model, hyps, W, H, scenario["proj"], sd, tau).tobytes()
    ed = api.scene_edge_distance(sd, W, H, jump, radius)
    con = api.score_contours(model, hyps, W, H, scenario["proj"], sd, tau, jump, ed)[1]
    for a, b in (("contour", "contour"), ("used", "hit"), ("occluded", "occluded"), ("miss", "miss")):
        assert np.array_equal(fit[a], con[b]), (a, b)
    for f in ("contour", "used", "occluded", "miss"):               # every class occurs, or the test proves little
        assert fit[f].sum() > 0, f
    assert (fit["sum_d2"].sum() > 0) == (radius > 0)
    # the same bytes on a second call, with and without the scores
    again = api.contour_information(model, hyps, W, H, scenario["proj"], scenario["K"], sd, tau, jump, nd, want_scores=False)
    assert again[0] is None and again[1].tobytes() == fit.tobytes() and again[2].tobytes() == info.tobytes()
    # a record does not depend on what else is in the batch
    sub = api.contour_information(model, hyps[5:12][::-1], W, H, scenario["proj"], scenario["K"], sd, tau, jump, nd)
    assert sub[1].tobytes() == fit[5:12][::-1].tobytes() and sub[2].tobytes() == info[5:12][::-1].tobytes()


@pytest.mark.parametrize("roi", ROIS)
def test_roi_windows(gpu, model, scenario, hyps, scene, centre, roi):
    cm, rho = centre
    poses = hyps[:16]
    N = _nearest(scene, 10, 3)
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"], roi)
    cs = CF.centers(poses, cm)
    refs = CF.fit_records(r, scene, N, 10, 10, scenario["K"], cs, rho, roi)
    for dt in (np.int32, np.uint16):
        s = _as(scene, dt)
        nd = api.scene_edge_nearest(s, W, H, 10, 3)
        _, fit, info = api.contour_information(model, poses, W, H, scenario["proj"], scenario["K"], s, 10, 10, nd, roi=roi)
        assert_records(fit, info, refs, cs, rho, (roi, dt))
    assert fit["used"].sum() > 0


def test_hypothesis_across_the_frame_border(gpu, model, scenario, scene, centre):
    cm, rho = centre
    base = scenario["poses"][1]
    poses = np.stack([base.copy() for _ in range(5)])
    poses[0, 0, 3] -= 175.0
    poses[1, 0, 3] += 170.0
    poses[2, 1, 3] -= 135.0
    poses[3, 1, 3] += 125.0
    poses[4, 0, 3] -= 185.0
    poses[4, 1, 3] += 110.0
    r = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    assert all((b > 0).sum() > 5 for b in (r[0][:, 0], r[1][:, W - 1], r[2][0, :], r[3][H - 1, :], r[4][:, 0], r[4][H - 1, :]))
    N = _nearest(scene, 10, 3)
    cs = CF.centers(poses, cm)
    refs = CF.fit_records(r, scene, N, 5, 10, scenario["K"], cs, rho)
    nd = api.scene_edge_nearest(scene, W, H, 10, 3)
    _, fit, info = api.contour_information(model, poses, W, H, scenario["proj"], scenario["K"], scene, 5, 10, nd)
    assert_records(fit, info, refs, cs, rho, "border")


def test_wide_tall_box_beside_a_single_pixel(gpu):
    """A box wider than 64 columns and taller than 16 rows (several strips, several workgroups, whose partial sums are added in block order) next to
    a hypothesis whose render is one pixel, and one that renders nothing."""
    w, h = 200, 90
    K = np.array([100.0, 0, 99.5, 0, 100.0, 44.5, 0, 0, 1], F32)
    proj = api.compute_proj(K, w, h)
    big = np.array([[-700, -300, 0], [700, -300, 0], [700, 300, 0], [-700, 300, 0]], F32)
    dot = np.array([[-4, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]], F32)      # under one pixel wide: it covers one pixel centre where it stands
    tris = lambda q: np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]], [q[0], q[2], q[1]], [q[0], q[3], q[2]]], F32)
    pose = np.eye(4, dtype=F32)
    pose[:3, 3] = [30.0, -20.0, 1000.0]
    off = pose.copy()
    off[0, 3] = 1.0e6
    small = pose.copy()
    small[:2, 3] = [35.0, -25.0]
    meshes, idx, poses = [tris(big), tris(dot)], np.array([0, 1, 0]), np.stack([pose, small, off])
    r = np.concatenate([O.render(meshes[m], poses[i:i + 1], w, h, proj) for i, m in enumerate(idx)])
    boxes = [np.argwhere(x > 0) for x in r]
    assert np.ptp(boxes[0][:, 1]) + 1 > 64 and np.ptp(boxes[0][:, 0]) + 1 > 16 and len(boxes[1]) == 1 and len(boxes[2]) == 0
    rng = np.random.default_rng(4)
    scene = np.where(r[0] > 0, 1000, 1200)
    scene = np.roll(scene, (3, -2), (0, 1)).astype(np.int32)       # the same silhouette a few pixels off: every contour pixel finds a scene edge
    scene[rng.random(scene.shape) < 0.02] = 0
    N = CF.nearest_ref(scene, 10, 6)
    cms, rad = np.zeros((2, 3), F32), np.array([0.5, 0.01], F32)
    nd = api.scene_edge_nearest(scene, w, h, 10, 6)
    _, fit, info = api.contour_information_multi(meshes, idx, poses, w, h, proj, K, scene, 5, 10, nd, centers=cms, radii=rad)
    for i in range(3):
        cs = CF.centers(poses[i:i + 1], cms[idx[i]])
        assert_records(fit[i:i + 1], info[i:i + 1], CF.fit_records(r[i:i + 1], scene, N, 5, 10, K, cs, rad[idx[i]]), cs, rad[idx[i]], i)
    assert fit["contour"].tolist()[1:] == [1, 0] and fit["used"][0] > 300 and fit["used"][2] == 0
    assert not I.flat_sums(info[2]).any() and info[2]["rho"] == F32(0.5)      # an empty render: all zero, c and rho as given


def test_no_scene_edge_within_reach(gpu, model, scenario, hyps, centre):
    """A flat scene without an edge: contour > 0, used == 0, every sum zero, c and rho as given."""
    cm, rho = centre
    flat = np.full((H, W), 700, np.int32)
    nd = api.scene_edge_nearest(flat, W, H, 10, 8)
    assert (nd.to_host() == api.EDGE_NONE).all()
    _, fit, info = api.contour_information(model, hyps[:4], W, H, scenario["proj"], scenario["K"], flat, 5, 10, nd)
    assert (fit["contour"] > 0).all() and not fit["used"].any() and not fit["sum_d2"].any()
    assert np.array_equal(fit["contour"], fit["occluded"] + fit["miss"])
    for o, c in zip(info, CF.centers(hyps[:4], cm)):
        assert not I.flat_sums(o).any() and np.array_equal(o["c"], c) and o["rho"] == F32(rho) and o["n_points"] > 0 and o["n_valid"] == 0
    empty = api.contour_information(model, np.zeros((0, 4, 4), F32), W, H, scenario["proj"], scenario["K"], flat, 5, 10, nd)
    assert len(empty[1]) == 0 and len(empty[2]) == 0


def test_chunked_batch_matches_small_batches(gpu, model, centre):
    """The 8192 x 2048 frame of test_contour_gpu.py: a chunk of the depth workspace holds 64 hypotheses, so 70 span two chunks."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], F32)
    proj = api.compute_proj(K, Wb, Hb)
    poses = synth.hypotheses(70, seed=9)
    scene = api.render_host(model, synth.scene_pose()[None], Wb, Hb, proj)[0]
    sd = api.DeviceVector.from_host(np.ascontiguousarray(scene, np.int32).reshape(-1))
    nd = api.scene_edge_nearest(sd, Wb, Hb, 10, 16)
    whole = api.contour_information(model, poses, Wb, Hb, proj, K, sd, 4, 10, nd)
    parts = [api.contour_information(model, poses[i:i + 25], Wb, Hb, proj, K, sd, 4, 10, nd) for i in range(0, 70, 25)]
    for k in range(3):
        assert whole[k].tobytes() == np.concatenate([p[k] for p in parts]).tobytes(), k
    assert (whole[1]["contour"] > 0).all() and whole[1]["used"].sum() > 0 and whole[2]["H"].any()


def test_batch_of_two_box_launches(gpu):
    """32768 + 5 hypotheses in one depth chunk: the launches over their boxes are split in two.  Every record is its pose's, the ones behind the split
    included.  Behind the split every hypothesis takes the next pose (seam_cases.seam_index): the first eight records are held to the reference, and
    every other one to the record of its pose among them, so hypothesis 32768 + j never expects hypothesis j's."""
    c = launch_split_case()
    idx = seam_index(c["P"], 8)
    assert np.array_equal(idx[:8], np.arange(8))
    poses = c["poses"][idx]
    K = np.array([60.0, 0, 23.5, 0, 60.0, 15.5, 0, 0, 1], F32)
    cm, rho = np.zeros(3, F32), 0.08
    nd = api.scene_edge_nearest(c["scene"], c["W"], c["H"], c["jump"], 3)
    N = CF.nearest_ref(c["scene"], c["jump"], 3)
    scores, fit, info = api.contour_information(c["tris"], poses, c["W"], c["H"], c["proj"], K, c["scene"], c["tau"], c["jump"], nd, center=cm, radius=rho)
    cs = CF.centers(c["poses"], cm)
    assert_records(fit[:8], info[:8], CF.fit_records(c["renders"], c["scene"], N, c["tau"], c["jump"], K, cs, rho), cs, rho, "split")
    for rec in (scores, fit, info):
        assert_seam_visible(rec[:8], idx)
        assert_records_take(rec, rec[:8], idx)
    assert scores[:8].tobytes() == c["scores"].tobytes() and fit["used"][:8].sum() > 0


def test_multi_mesh_matches_single_mesh_calls(gpu, scenario, hyps, scene):
    t = scenario["tris"]
    meshes = [np.ascontiguousarray(t * F32(0.7 + 0.1 * k)) for k in range(3)] + [np.zeros((0, 3, 3), F32)]
    idx = np.random.default_rng(3).permutation(np.repeat(np.arange(4), 8))
    cms = np.array([[0, 0, 0], [5, -3, 2], [-4, 1, 9], [0, 0, 0]], F32)
    rad = np.array([0.1, 0.12, 0.14, 0.2], F32)
    nd = api.scene_edge_nearest(scene, W, H, 10, 4)
    sc, fit, info = api.contour_information_multi(meshes, idx, hyps, W, H, scenario["proj"], scenario["K"], scene, 5, 10, nd, centers=cms, radii=rad)
    for m in range(4):
        sel = np.flatnonzero(idx == m)
        one = api.contour_information(meshes[m], hyps[sel], W, H, scenario["proj"], scenario["K"], scene, 5, 10, nd, center=cms[m], radius=float(rad[m]))
        assert sc[sel].tobytes() == one[0].tobytes() and fit[sel].tobytes() == one[1].tobytes() and info[sel].tobytes() == one[2].tobytes(), m
    assert (fit["contour"][idx == 3] == 0).all() and (fit["used"][idx != 3] > 0).all()


def test_private_context_gives_the_same_records(gpu, model, scenario, hyps, scene):
    nd = api.scene_edge_nearest(scene, W, H, 10, 3)
    shared = api.contour_information(model, hyps, W, H, scenario["proj"], scenario["K"], scene, 5, 10, nd)
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                mine = api.scene_edge_nearest(scene, W, H, 10, 3)
                box["nd"] = mine.to_host()
                box["out"] = api.contour_information(model, hyps, W, H, scenario["proj"], scenario["K"], scene, 5, 10, mine)
                mine.free()
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert np.array_equal(box["nd"], nd.to_host())
    for k in range(3):
        assert box["out"][k].tobytes() == shared[k].tobytes()


def test_scene_and_nearest_map_are_read_on_every_call(gpu, model, scenario, hyps, scene, renders, centre):
    cm, rho = centre
    poses, r = hyps[:8], renders[:8]
    cs = CF.centers(poses, cm)
    s2 = np.ascontiguousarray(scenario["depth"][1], np.int32)
    N1, N2 = _nearest(scene, 10, 3), CF.nearest_ref(s2, 10, 3)
    sd = api.DeviceVector.from_host(np.ascontiguousarray(scene).reshape(-1))
    nd = api.scene_edge_nearest(sd, W, H, 10, 3)

    def check(sc, N, what):
        _, fit, info = api.contour_information(model, poses, W, H, scenario["proj"], scenario["K"], sd, 5, 10, nd)
        assert_records(fit, info, CF.fit_records(r, sc, N, 5, 10, scenario["K"], cs, rho), cs, rho, what)
    check(scene, N1, "as made")
    raw_h2d(nd.data(), N2)                                          # the map overwritten behind the library's back
    check(scene, N2, "other map")
    raw_h2d(sd.data(), s2)                                          # ... and the scene
    check(s2, N2, "other scene")


# ---- the host-only calls against the device's records, and the loop ------------------------------------------------------------------------------
def test_step_and_eig_on_device_records(gpu, model, scenario, hyps, scene, renders, gscenes, centre):
    cm, rho = centre
    poses = hyps[:8]
    surf, eig_dev, _ = api.pose_information(model, poses, W, H, scenario["proj"], scenario["K"], gscenes["proj"])
    eig = api.information_eig(surf)
    for a, b in zip(eig, eig_dev):                                  # the host's Jacobi against the device's, on the device's own records
        top = b["lambda"][5]
        Va, Vb = np.asarray(a["V"]).reshape(6, 6), np.asarray(b["V"]).reshape(6, 6)
        assert np.abs(a["lambda"] - b["lambda"]).max() <= 1e-12 * top and np.abs(Va - Vb).max() <= 1e-12 and a["sweeps"] == b["sweeps"]
    nd = api.scene_edge_nearest(scene, W, H, 10, 4)
    _, fit, con = api.contour_information(model, poses, W, H, scenario["proj"], scenario["K"], scene, 5, 10, nd)
    both = api.combine_information(surf, con, 1.0, 0.5)
    e2 = api.information_eig(both)
    new, delta, rank = api.information_step(both, e2, poses, 1e-6)
    cs = CF.centers(poses, cm)
    refs = CF.fit_records(renders[:8], scene, _nearest(scene, 10, 4), 5, 10, scenario["K"], cs, rho)
    for i in range(8):                                              # one step from the same pose: the reference's contour record, the device's surface record
        want = CF.combine(surf[i], 1.0, CF.info_of(refs[i], cs[i], rho), 0.5)
        lam, V, _ = CF.jacobi(want["H"])
        _, wdelta, wrank = CF.step(want["g"], want["c"], want["rho"], lam, V, 1e-6, poses[i])
        assert rank[i] == wrank == 6
        assert np.abs(delta[i] - wdelta).max() <= 1e-9 * np.abs(wdelta).max(), i
    assert np.abs(new - poses).max() > 0


def test_refine_contours_on_the_plate(gpu):
    """The host test's case through the library: render, surface and contour records on the device, combine, Jacobi and step on the host.  Not
    compared pose for pose with the reference loop: a one-ulp pose difference may move a rendered pixel."""
    P = CF.PLATE
    Wp, Hp, K = P["W"], P["H"], P["K"]
    tris, proj = CF.plate_tris(), api.compute_proj(K, Wp, Hp)
    true, start = CF.plate_poses()
    scene = CF.plate_scene(api.render_host(tris, true[None], Wp, Hp, proj)[0])
    assert np.array_equal(scene, CF.plate_scene(O.render(tris, true[None], Wp, Hp, O.compute_proj(K, Wp, Hp))[0]))
    surface = api.Scene_projective().init_Scene_projective_cuda(scene, K, width=Wp, height=Hp, max_dist_diff=P["max_dist_diff"])
    nd = api.scene_edge_nearest(scene, Wp, Hp, P["jump"], P["radius"])
    cm = np.zeros(3, F32)
    info0, eig0, sizes = api.pose_information(tris, start[None], Wp, Hp, proj, K, surface, center=cm, radius=P["rho"])
    assert sizes[0] > 1000 and info0[0]["n_valid"] > 500
    poses, hist = api.refine_contours(tris, start[None], Wp, Hp, proj, K, surface, scene, nd, P["tau"], P["jump"], iterations=P["iterations"],
                                      weight=P["weight"], min_ratio=P["min_ratio"], min_used=P["min_used"], center=cm, radius=P["rho"])
    assert hist["rank"].shape == (P["iterations"], 1) and (hist["used"] >= P["min_used"]).all()
    assert_plate_conditions(true, start, poses[0], np.asarray(eig0[0]["lambda"]), int(hist["rank"][0, 0]), "refine_contours")
    assert hist["rms_px"][-1, 0] < hist["rms_px"][0, 0] / 4.0
    many, h2 = api.refine_contours_multi([tris, tris], [1, 0, 1], np.stack([start, true, start]), Wp, Hp, proj, K, surface, scene, nd, P["tau"], P["jump"],
                                         iterations=P["iterations"], weight=P["weight"], min_ratio=P["min_ratio"], min_used=P["min_used"],
                                         centers=[cm, cm], radii=[P["rho"], P["rho"]])
    assert many[0].tobytes() == poses[0].tobytes() == many[2].tobytes() and CF.plate_errors(many[1], true)[0] < 0.5
    frozen, h3 = api.refine_contours(tris, start[None], Wp, Hp, proj, K, surface, scene, nd, P["tau"], P["jump"], iterations=2, weight=1.0, min_ratio=1e-6,
                                     min_used=10**6, center=cm, radius=P["rho"])
    assert frozen[0].tobytes() == start.tobytes() and (h3["used"] > 0).all()      # fewer used pixels than min_used: the pose stays
