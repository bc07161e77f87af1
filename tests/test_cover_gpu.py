"""GPU tests (-m gpu) of pr_score_cover / pr_score_cover_multi: the scores are pr_score_poses' bytes (and verify_ref.score_ref's), and the
records, the frame record and the selected list equal the cover rule in Python integers over the oracle's renders (tests/cover_ref.py) byte
for byte -- tiny batches and one larger than a wavefront, int32 and uint16 scenes, word and box edges, pathological hypotheses, partial and
reversed orders, the cap, ROI windows, several depth chunks, mixed batches, a call between submit and wait, a private context, the planted
frame, the straddler, a batch beyond PR_OVERLAP_MAX_POSES and one of two launches over its boxes."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O
from cover_ref import (ACCEPTED, EMPTY, KEEP_ALL, NOT_IN_ORDER, PLANTED_FRESH, REJ_CAP, REJ_THRESHOLD, STRADDLER_SUPPORT, STRADDLER_TAU,
                       assert_cover_equal, cover_ref, straddler_frame, supports_of)
from gpu_common import W, H, pathological_hypotheses
from pose_refine_amd import _lib, api, synth
from select_ref import PLANTED_SELECTION, planted_frame, shift
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import assert_scores_equal, launch_split_case, score_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hyps():
    return synth.hypotheses(256)                                  # configs[1] sampler


@pytest.fixture(scope="module")
def noisy_scene(scenario):
    """test_select_gpu.py's scene: depth[1] with holes, +-k mm perturbations, a wall behind and clutter in front of the object."""
    rng = np.random.default_rng(20)
    d = scenario["depth"][1].astype(np.int64)
    d = d + np.where(rng.random(d.shape) < 0.4, rng.integers(-25, 26, d.shape), 0) * (d > 0)
    bg = d == 0
    d[bg & (rng.random(d.shape) < 0.5)] = 900
    d[bg & (rng.random(d.shape) < 0.1)] = 150
    d[rng.random(d.shape) < 0.08] = 0
    return d.astype(np.int32)


@pytest.fixture(scope="module")
def renders64(scenario, hyps):
    """The oracle's renders of the first 65 hypotheses, shared (and left unchanged) by the tests that walk them."""
    return O.render(scenario["tris"], hyps[:65], W, H, scenario["proj"])


RULES = [((1, 2), 1, None), ((0, 1), 1, None), ((1, 50), 40, None), ((1, 1), 1, None), ((0, 1), 1, 2)]


def _check(call, sup, n_pix, want_sc, order, frac, min_new, max_keep):
    """One device call against the references: returns (scores, cover, frame, selected)."""
    sc, cov, frame, sel = call(order, frac, min_new, max_keep)
    assert_scores_equal(sc, want_sc)
    assert np.array_equal(cov["support"], sc["inlier"])
    assert_cover_equal((cov, frame, sel), cover_ref(sup, n_pix, order, *frac, min_new, KEEP_ALL if max_keep is None else max_keep))
    return sc, cov, frame, sel


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("P", [1, 2, 3, 65])
def test_tiny_batches_and_one_beyond_a_wavefront(gpu, model, scenario, hyps, noisy_scene, renders64, P, dtype):
    """P = 65: more undecided hypotheses than one wavefront's ballot in the commit kernel.  (0, 1) with min_new = 1 accepts many of them:
    more rounds than one batch of enqueued rounds, so the finished word is read back in between."""
    scene = np.ascontiguousarray(noisy_scene.astype(dtype))
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    poses, renders = hyps[1:1 + P] if P < 4 else hyps[:P], renders64[1:1 + P] if P < 4 else renders64[:P]
    most = 0
    for tau in (0, 5, 40):
        want_sc = score_ref(renders, scene, tau)
        sup, n = supports_of(renders, scene, tau)
        assert api.score_poses(model, poses, W, H, scenario["proj"], sd, tau).tobytes() == want_sc.tobytes()
        order = api.rank_hypotheses(want_sc)
        for frac, min_new, max_keep in RULES:
            sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], sd, tau, o, f, m, k), sup, n, want_sc,
                                         order, frac, min_new, max_keep)
            most = max(most, len(sel))
    assert most >= (1 if P < 4 else 6)                           # several rounds were walked


def _quad(x0, x1, y0, y1, z):
    return np.array([[[x0, y0, z], [x1, y0, z], [x1, y1, z]], [[x0, y0, z], [x1, y1, z], [x0, y1, z]]], np.float32)


def test_word_and_box_edges(gpu, scenario):
    """A 600 x 400 frame (the last 64-pixel word of a row is cut at pixel 599), the hypotheses of test_select_gpu's odd-width test -- boxes
    inside one word, across a word boundary, cut by every edge of the frame -- and four slivers rendered at 1000 mm: one pixel wide inside
    word 8, one pixel high across it (the two share exactly one pixel), one that reaches one pixel into word 8, one in the last column."""
    Wo, Ho = 600, 400
    K = np.array([572.4114, 0, 300, 0, 573.57043, 200, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Wo, Ho)
    S = synth.scene_pose()

    def at(x, y, z):
        p = S.copy()
        p[:3, 3] = (x, y, z)
        return p

    one_word = [at(x, y, 3000.0) for x in (-63.0, -58.0, -70.0) for y in (0.0, 12.0)]
    straddle = [at(x, 5.0, 3000.0) for x in (100.0, 105.0, 270.0)] + [at(-20.0, 0.0, 2000.0), at(-30.0, 8.0, 2000.0)]
    edges = [at(380.0, 0.0, 800.0), at(385.0, 10.0, 800.0), at(300.0, 100.0, 700.0), at(-380.0, 0.0, 800.0), at(-375.0, -8.0, 800.0),
             at(0.0, -260.0, 800.0), at(10.0, -255.0, 800.0), at(0.0, 262.0, 800.0), at(1560.0, 0.0, 3000.0), at(1555.0, 4.0, 3000.0)]
    near = [at(0.0, 0.0, 250.0), at(5.0, 5.0, 260.0), at(20.0, 20.0, 320.0)]
    obj_poses = np.stack(one_word + straddle + edges + near).astype(np.float32)
    z, px, py = 1000.0, 1000.0 / 572.4114, 1000.0 / 573.57043
    slivers = [_quad(220.3 * px, 221.3 * px, -160.0 * py, -139.7 * py, z),     # column 521, 21 rows high
               _quad(210.0 * px, 230.3 * px, -149.7 * py, -148.7 * py, z),     # one row, columns 510 .. 530: crosses the column
               _quad(192.3 * px, 212.3 * px, -170.7 * py, -169.7 * py, z),     # one row, columns 493 .. 512: one pixel into word 8
               _quad(298.6 * px, 301.0 * px, -165.2 * py, -154.7 * py, z)]     # the last column
    meshes = [scenario["tris"]] + slivers
    idx = np.concatenate([np.zeros(len(obj_poses), np.int64), 1 + np.arange(4)])
    poses = np.concatenate([obj_poses, np.broadcast_to(np.eye(4, dtype=np.float32), (4, 4, 4))]).astype(np.float32)
    renders = np.concatenate([O.render(scenario["tris"], obj_poses, Wo, Ho, proj)] +
                             [O.render(m, np.eye(4, dtype=np.float32)[None], Wo, Ho, proj) for m in slivers])
    cols = [np.flatnonzero((r > 0).any(0)) for r in renders[-4:]]
    rows = [np.flatnonzero((r > 0).any(1)) for r in renders[-4:]]
    assert len(cols[0]) == 1 and len(rows[0]) == 21 and cols[0][0] >> 6 == 8                  # one pixel wide, inside one word
    assert len(rows[1]) == 1 and cols[1][0] < cols[0][0] < cols[1][-1]
    assert len(rows[2]) == 1 and cols[2][-1] == 512 and cols[2][0] >> 6 == 7                  # spans the word boundary by one pixel
    assert cols[3].tolist() == [Wo - 1]                                                       # ends in the last column
    r = renders.astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    rng = np.random.default_rng(3)
    quiet = (renders[-4:] > 0).any(0)                             # the slivers' pixels stay as rendered
    scene = scene + np.where(rng.random(scene.shape) < 0.3, rng.integers(-6, 7, scene.shape), 0) * (scene > 0) * ~quiet
    scene[(rng.random(scene.shape) < 0.05) & ~quiet] = 0
    n_obj = len(obj_poses)
    for dt in (np.int32, np.uint16):
        sce = np.ascontiguousarray(scene.astype(dt))
        for tau in (0, 4, 3000):
            want_sc = score_ref(renders, sce, tau)
            sup, n = supports_of(renders, sce, tau)
            both = np.intersect1d(sup[n_obj], sup[n_obj + 1])
            assert len(both) == 1 and len(sup[n_obj]) == 21 and len(sup[n_obj + 1]) == 21    # two supports that share exactly one pixel
            for order in (api.rank_hypotheses(want_sc), np.arange(len(poses))[::-1], np.r_[n_obj:n_obj + 4, 0:n_obj]):
                for frac, min_new, max_keep in RULES[:3] + [((20, 21), 1, None), ((21, 21), 1, None)]:
                    sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover_multi(meshes, idx, poses, Wo, Ho, proj, sce, tau, o, f, m, k),
                                                 sup, n, want_sc, order, frac, min_new, max_keep)
    # the slivers walked first, the bound at one shared pixel: 20 of 21 new pixels pass (20, 21) and fail (21, 21)
    s0, s1 = n_obj, n_obj + 1
    _, cov, _, sel = api.score_cover_multi(meshes, idx, poses, Wo, Ho, proj, sce, 4, [s0, s1], (20, 21))
    assert sel.tolist() == [s0, s1] and cov["fresh"][[s0, s1]].tolist() == [21, 20]
    _, cov, _, sel = api.score_cover_multi(meshes, idx, poses, Wo, Ho, proj, sce, 4, [s0, s1], (21, 21))
    assert sel.tolist() == [s0] and cov["fresh"][s1] == 20 and cov["state"][s1] == REJ_THRESHOLD


def test_pathological_hypotheses_and_repeated_poses(gpu, model, scenario, noisy_scene):
    """NaN / infinite / zero matrices, off-frame, behind the camera, a giant, a speck, one entirely behind the scene's surface (every pixel
    occluded): support 0, state EMPTY, and the rest as without them.  The same pose four times: the first is accepted, the copies are
    rejected with fresh == 0."""
    bad, idx_bad = pathological_hypotheses(synth.hypotheses(40, seed=3))
    hidden = synth.scene_pose() + shift(0, 0, 150)                # behind the object the scene shows
    poses = np.concatenate([bad, hidden[None], np.repeat(synth.scene_pose()[None], 4, 0)]).astype(np.float32)
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    tau = 10
    want_sc = score_ref(renders, noisy_scene, tau)
    sup, n = supports_of(renders, noisy_scene, tau)
    assert want_sc["visible"][40] > 1000 and want_sc["inlier"][40] == 0 and want_sc["occluded"][40] > 1000
    call = lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], noisy_scene, tau, o, f, m, k)
    for order in (np.arange(len(poses)), api.rank_hypotheses(want_sc), np.arange(len(poses))[::-1]):
        for frac, min_new, max_keep in RULES:
            sc, cov, frame, sel = _check(call, sup, n, want_sc, order, frac, min_new, max_keep)
            empty = [i for i in idx_bad + [40] if sc["inlier"][i] == 0]
            assert len(empty) >= 9 and (cov["state"][empty] == EMPTY).all() and not cov["fresh"][empty].any()
    sc, cov, frame, sel = _check(call, sup, n, want_sc, np.array([41, 42, 43, 44]), (0, 1), 1, None)
    assert sel.tolist() == [41] and cov["state"][41:45].tolist() == [ACCEPTED] + [REJ_THRESHOLD] * 3 and cov["fresh"][41:45].tolist() == [cov["support"][41], 0, 0, 0]
    # an empty mesh: nothing has support
    none = api.Model(tris=np.zeros((0, 3, 3), np.float32))
    sc, cov, frame, sel = api.score_cover(none, poses[:7], W, H, scenario["proj"], noisy_scene, tau, np.arange(7))
    assert len(sel) == 0 and (cov["state"] == EMPTY).all() and not sc["visible"].any() and frame["claimed"] == 0


def test_partial_and_reversed_orders_and_the_cap(gpu, model, scenario, hyps, noisy_scene, renders64):
    poses, renders = hyps[:65], renders64
    tau = 5
    want_sc = score_ref(renders, noisy_scene, tau)
    sup, n = supports_of(renders, noisy_scene, tau)
    rank = api.rank_hypotheses(want_sc)
    call = lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], noisy_scene, tau, o, f, m, k)
    free = len(_check(call, sup, n, want_sc, rank, (0, 1), 1, None)[3])
    assert free >= 6
    for order in (rank[::2], rank[::-1], rank[5:40][::-1], rank[:1], np.zeros(0, np.int64)):
        for max_keep in (None, 0, 1, 3, free, free + 1):
            sc, cov, frame, sel = _check(call, sup, n, want_sc, order, (0, 1), 1, max_keep)
            outside = np.setdiff1d(np.arange(65), order)
            assert (cov["state"][outside] == NOT_IN_ORDER).all() and (cov["state"][order] != NOT_IN_ORDER).all()
            if max_keep is not None and max_keep < 3 and len(order) > 10:
                assert len(sel) == max_keep and (cov["state"][order] == REJ_CAP).sum() >= 3      # fewer kept than would pass
            if max_keep == 0:
                assert np.array_equal(cov["fresh"], cov["support"] * (cov["state"] != EMPTY))     # nothing claimed


@pytest.mark.parametrize("roi", [(200, 150, 200, 180), (321, 200, 62, 90)])
def test_roi(gpu, model, scenario, hyps, noisy_scene, roi):
    poses = hyps[:64]
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"], roi)
    for dt in (np.int32, np.uint16):
        scene = np.ascontiguousarray(noisy_scene.astype(dt))
        want_sc = score_ref(renders, scene, 10, roi)
        sup, n = supports_of(renders, scene, 10, roi)
        assert api.score_poses(model, poses, W, H, scenario["proj"], scene, 10, roi=roi).tobytes() == want_sc.tobytes()
        for frac, min_new, max_keep in RULES:
            sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], scene, 10, o, f, m, k, roi=roi), sup, n,
                                         want_sc, api.rank_hypotheses(want_sc), frac, min_new, max_keep)
    assert frame["claimed"] > 0


def test_two_depth_chunks(gpu, model, scenario):
    """An 8192 x 2048 frame: 66 hypotheses are two chunks of the depth workspace (64 + 2).  The planes, boxes and walk state of the first
    chunk must survive the second, and the walk must cross the chunks.  A ROI window around the hypotheses keeps the oracle's renders small;
    the device still sizes its chunks by the frame."""
    Wb, Hb = 8192, 2048
    K = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    proj = api.compute_proj(K, Wb, Hb)
    roi = (3500, 500, 1200, 1050)
    poses = synth.hypotheses(66, seed=9)
    scene = O.render(scenario["tris"], synth.scene_pose()[None], Wb, Hb, proj)[0]
    rng = np.random.default_rng(2)
    scene = np.where(rng.random(scene.shape) < 0.1, 0, scene + rng.integers(-8, 9, scene.shape) * (scene > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    renders = O.render(scenario["tris"], poses, Wb, Hb, proj, roi)
    assert sum(bool((r[[0, -1]] > 0).any() or (r[:, [0, -1]] > 0).any()) for r in renders) < 10      # the window holds most hypotheses whole
    want_sc = score_ref(renders, scene, 4, roi)
    sup, n = supports_of(renders, scene, 4, roi)
    for order in (api.rank_hypotheses(want_sc), np.arange(66)[::-1]):
        sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover(model, poses, Wb, Hb, proj, sd, 4, o, f, m, k, roi=roi), sup, n, want_sc, order,
                                     (0, 1), 1, None)
    assert (sel >= 64).any() and (sel < 64).any() and len(sel) >= 4


def _rigid(tris, angle, t):
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    return np.ascontiguousarray((tris.reshape(-1, 3) @ R.T + np.asarray(t, np.float32)).astype(np.float32).reshape(-1, 3, 3))


def test_mixed_batch_of_two_meshes_interleaved(gpu, model, scenario, hyps, noisy_scene, renders64):
    t = scenario["tris"]
    meshes = [t, _rigid(t, 0.3, (4.0, -3.0, 2.0))]
    poses = hyps[:64]
    idx = np.arange(64) % 2
    rr = renders64[:64].copy()
    rr[1::2] = O.render(meshes[1], poses[1::2], W, H, scenario["proj"])
    tau = 10
    want_sc = score_ref(rr, noisy_scene, tau)
    sup, n = supports_of(rr, noisy_scene, tau)
    call = lambda o, f, m, k: api.score_cover_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, tau, o, f, m, k)
    for order in (api.rank_hypotheses(want_sc), np.arange(64)[::-1], np.arange(1, 64, 2)):
        for frac, min_new, max_keep in RULES:
            sc, cov, frame, sel = _check(call, sup, n, want_sc, order, frac, min_new, max_keep)
    assert sc.tobytes() == api.score_poses_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, tau).tobytes()
    # walking one mesh's hypotheses alone in a mixed batch is the single-mesh call on them, record for record
    odd = np.arange(1, 64, 2)
    for frac, min_new, max_keep in RULES:
        _, mcov, mframe, msel = api.score_cover_multi(meshes, idx, poses, W, H, scenario["proj"], noisy_scene, tau, odd, frac, min_new, max_keep)
        ssc, scov, sframe, ssel = api.score_cover(meshes[1], poses[odd], W, H, scenario["proj"], noisy_scene, tau, np.arange(32), frac, min_new, max_keep)
        assert ssc.tobytes() == sc[odd].tobytes() and scov.tobytes() == mcov[odd].tobytes() and sframe.tobytes() == mframe.tobytes()
        assert odd[ssel].tolist() == msel.tolist()
    # a mixed batch of one mesh is the single-mesh call
    one = api.score_cover(model, poses, W, H, scenario["proj"], noisy_scene, tau, np.arange(64), (0, 1))
    for ms, ix in (([model], np.zeros(64, np.int64)), ([t[:10], model], np.ones(64, np.int64))):
        got = api.score_cover_multi(ms, ix, poses, W, H, scenario["proj"], noisy_scene, tau, np.arange(64), (0, 1))
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, one))


@pytest.mark.parametrize("solve", [api.SOLVE_DEVICE, api.SOLVE_HOST])
def test_cover_between_submit_and_wait(gpu, model, scenario, hyps, gscenes, noisy_scene, solve):
    before = api.get_option("solve")
    api.set_option("solve", solve)
    try:
        crit = api.ICPConvergenceCriteria(0.0, 0.0, 20)
        order = np.arange(256)[::-1]
        alone_res, alone_sizes = api.refine_batch(model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        alone = api.score_cover(model, hyps, W, H, scenario["proj"], noisy_scene, 5, order, (0, 1))
        api.refine_submit(0, model, hyps, W, H, scenario["proj"], scenario["K"], gscenes["proj"], crit)
        mid = api.score_cover(model, hyps, W, H, scenario["proj"], noisy_scene, 5, order, (0, 1))
        res, sizes = api.refine_wait(0)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(mid, alone)) and len(mid[3]) >= 6
        assert np.array_equal(sizes, alone_sizes) and res.tobytes() == alone_res.tobytes()
    finally:
        api.set_option("solve", before)


def test_private_context_gives_the_same_bytes(gpu, model, scenario, hyps, noisy_scene):
    order = api.rank_hypotheses(api.score_poses(model, hyps, W, H, scenario["proj"], noisy_scene, 5))
    shared = api.score_cover(model, hyps, W, H, scenario["proj"], noisy_scene, 5, order, (0, 1))
    box = {}

    def work():
        try:
            api.init(0)
            api.thread_context(True)
            try:
                box["out"] = api.score_cover(model, hyps, W, H, scenario["proj"], noisy_scene, 5, order, (0, 1))
            finally:
                api.thread_context(False)
        except Exception as e:                                    # reported by the main thread
            box["err"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert "err" not in box, box.get("err")
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(box["out"], shared))
    # and a second call into the same workspaces, the batch reversed: the same walk
    again = api.score_cover(model, hyps[::-1], W, H, scenario["proj"], noisy_scene, 5, 255 - order, (0, 1))
    assert again[0].tobytes() == shared[0][::-1].tobytes() and again[1].tobytes() == shared[1][::-1].tobytes()
    assert again[2].tobytes() == shared[2].tobytes() and (255 - again[3]).tolist() == shared[3].tolist()


def test_arguments(gpu, model, scenario, hyps, noisy_scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(scenario["proj"], np.float32)
    roi0 = _lib.Roi(0, 0, 0, 0)
    # no hypotheses: PR_OK, *n_selected = 0 and nothing else written (null pointers allowed)
    n = C.c_uint32(9)
    assert lib.pr_score_cover(None, 0, None, 0, W, H, pj.ctypes.data, roi0, None, 1, 5, None, 0, 1, 2, 1, KEEP_ALL, None, None, None, None, C.byref(n)) == _lib.PR_OK
    assert n.value == 0
    assert lib.pr_score_cover_multi(None, 0, None, None, 0, W, H, pj.ctypes.data, roi0, None, 1, 5, None, 0, 1, 2, 1, KEEP_ALL, None, None, None, None, None) == _lib.PR_OK
    sc, cov, frame, sel = api.score_cover(model, np.zeros((0, 4, 4), np.float32), W, H, pj, noisy_scene, 5, [])
    assert len(sc) == 0 and len(cov) == 0 and len(sel) == 0
    # no order: scores as ever, everything NOT_IN_ORDER with fresh = support
    sc, cov, frame, sel = api.score_cover(model, hyps[:9], W, H, pj, noisy_scene, 5, [])
    assert sc.tobytes() == api.score_poses(model, hyps[:9], W, H, pj, noisy_scene, 5).tobytes() and len(sel) == 0 and frame["claimed"] == 0
    assert (cov["state"] == NOT_IN_ORDER).all() and np.array_equal(cov["fresh"], sc["inlier"]) and np.array_equal(cov["support"], sc["inlier"])
    # the rule's own checks and pr_score_poses': PR_ERR_INVALID, nothing written
    td = model.device_tris()
    pp = np.ascontiguousarray(hyps[:4], np.float32)
    sd = api.DeviceVector.from_host(noisy_scene.reshape(-1))

    def raw(order, num, den, tau=5, roi=roi0, null=()):
        od = np.ascontiguousarray(order, np.uint32)
        out = np.zeros(4, api.SCORE)
        cov = np.frombuffer(bytearray(b"\xee" * 64), _lib.COVER)
        frame = np.frombuffer(bytearray(b"\xee" * 16), _lib.COVER_FRAME)
        sel = np.full(8, 0xeeeeeeee, np.uint32)
        k = C.c_uint32(12345)
        a = dict(order=od.ctypes.data, scores=out.ctypes.data, cov=cov.ctypes.data, frame=frame.ctypes.data, sel=sel.ctypes.data, n=C.byref(k), scene=sd.data())
        for name in null:
            a[name] = None
        rc = lib.pr_score_cover(td.data(), td.size() // 9, pp.ctypes.data, 4, W, H, pj.ctypes.data, roi, a["scene"], 1, tau, a["order"], len(od), num, den, 1,
                                KEEP_ALL, a["scores"], a["cov"], a["frame"], a["sel"], a["n"])
        clean = not out["visible"].any() and cov.tobytes() == b"\xee" * 64 and frame.tobytes() == b"\xee" * 16 and (sel == 0xeeeeeeee).all() and k.value == 12345
        return rc, clean

    assert raw([0, 1, 2, 3], 1, 2) == (_lib.PR_OK, False)
    for args in (([0, 1], 1, 0), ([0, 1], 3, 2), ([0, 4], 1, 2), ([2, 1, 2], 1, 2), ([4294967295], 1, 2)):
        assert raw(*args) == (_lib.PR_ERR_INVALID, True), args
    assert raw([0, 1], 1, 2, tau=-1) == (_lib.PR_ERR_INVALID, True)
    assert raw([0, 1], 1, 2, roi=_lib.Roi(600, 0, 100, 100)) == (_lib.PR_ERR_INVALID, True)
    for name in ("order", "scores", "cov", "frame", "sel", "n", "scene"):
        assert raw([0, 1], 1, 2, null=(name,)) == (_lib.PR_ERR_INVALID, True), name
    with pytest.raises(api.PoseRefineError) as e:
        api.score_cover(model, hyps[:4], W, H, pj, noisy_scene, 5, [0, 0])
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_score_cover" in str(e.value) and "twice" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:
        api.score_cover_multi([model], [0, 0, 0, 0], hyps[:4], W, H, pj, noisy_scene, 5, [0], (1, 0))
    assert e.value.code == _lib.PR_ERR_INVALID and "new_den" in str(e.value)
    with pytest.raises(ValueError):
        api.score_cover_multi([model], [0, 0, 0, 1], hyps[:4], W, H, pj, noisy_scene, 5, [0])


def test_planted_frame_and_straddler_through_the_device(gpu, model, scenario):
    """The host test's figures from the device: the three planted instances with their recorded counts, and the straddler -- kept by the
    pairwise rule at (3, 5), dropped by the cover rule at (1, 10) with fresh == 0."""
    scene, poses = planted_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    for tau in (5, 10):
        want_sc = score_ref(renders, scene, tau)
        sup, n = supports_of(renders, scene, tau)
        order = api.rank_hypotheses(want_sc)
        sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], sd, tau, o, f, m, k), sup, n, want_sc, order,
                                     (1, 2), 1, None)
        fresh, claimed = PLANTED_FRESH[tau]
        assert sel.tolist() == PLANTED_SELECTION and cov["fresh"][sel].tolist() == fresh and frame["claimed"] == claimed
        # select_cover: the ranking and min_fraction applied for the caller
        for mf in (0.0, 0.5):
            s2, c2, f2 = api.select_cover(sc, model, poses, W, H, scenario["proj"], sd, tau, min_fraction=mf)
            assert s2.tolist() == PLANTED_SELECTION and f2["claimed"] == claimed
        assert api.select_cover(sc, model, poses, W, H, scenario["proj"], sd, tau, max_keep=2)[0].tolist() == PLANTED_SELECTION[:2]
    scene, poses = straddler_frame(O.render, scenario["tris"], W, H, scenario["proj"])
    renders = O.render(scenario["tris"], poses, W, H, scenario["proj"])
    sc, ov = api.score_overlap(model, poses, W, H, scenario["proj"], scene, STRADDLER_TAU)
    assert api.select_greedy([0, 1, 2], ov, 3, 5).tolist() == [0, 1, 2]
    sup, n = supports_of(renders, scene, STRADDLER_TAU)
    sc, cov, frame, sel = _check(lambda o, f, m, k: api.score_cover(model, poses, W, H, scenario["proj"], scene, STRADDLER_TAU, o, f, m, k), sup, n,
                                 score_ref(renders, scene, STRADDLER_TAU), np.arange(3), (1, 10), 1, None)
    assert sel.tolist() == [0, 1] and cov["support"][2] == STRADDLER_SUPPORT and cov["fresh"][2] == 0 and cov["state"][2] == REJ_THRESHOLD


def test_more_hypotheses_than_the_overlap_matrix_allows(gpu, scenario):
    """4097 hypotheses of a thinned mesh on a 128 x 96 frame: PR_OVERLAP_MAX_POSES does not apply to the cover walk."""
    Ws, Hs, P = 128, 96, api.OVERLAP_MAX_POSES + 1
    K = np.array([114.48, 0, 64, 0, 114.71, 48, 0, 0, 1], np.float32)
    proj = O.compute_proj(K, Ws, Hs)
    tris = np.ascontiguousarray(scenario["tris"][::16])
    poses = synth.hypotheses(P, seed=31)
    rng = np.random.default_rng(5)
    poses[:, :2, 3] += rng.uniform(-120, 120, (P, 2)).astype(np.float32)      # spread over the frame
    renders = np.concatenate([O.render(tris, poses[i:i + 512], Ws, Hs, proj) for i in range(0, P, 512)])
    r = renders[::64].astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    scene = (scene + rng.integers(-4, 5, scene.shape) * (scene > 0)).astype(np.int32)
    want_sc = score_ref(renders, scene, 6)
    sup, n = supports_of(renders, scene, 6)
    m = api.Model(tris=tris)
    with pytest.raises(api.PoseRefineError):
        api.score_overlap(m, poses, Ws, Hs, proj, scene, 6)      # the matrix route refuses the batch
    for frac, min_new, max_keep in (((0, 1), 1, None), ((1, 2), 1, None), ((0, 1), 1, 5)):
        sc, cov, frame, sel = _check(lambda o, f, mn, k: api.score_cover(m, poses, Ws, Hs, proj, scene, 6, o, f, mn, k), sup, n, want_sc,
                                     api.rank_hypotheses(want_sc), frac, min_new, max_keep)
    assert (sel < 5000).all() and frame["n_selected"] == 5 and (cov["state"] == REJ_CAP).sum() > 100


@pytest.mark.parametrize("reverse", [False, True])
def test_batch_of_two_box_launches(gpu, reverse):
    """verify_ref.launch_split_case at 32768 + 5 hypotheses: the launches over the boxes are split in two, each with its own support bits,
    planes and records.  In natural order the first of every pose claims its pixels; reversed, the walk starts behind the split.  The
    selected list and every record are the reference's, the states of the hypotheses behind the split included.  Behind the split every
    hypothesis takes the next pose (seam_cases.seam_index), and the reference is recomputed from the stack so indexed: hypothesis 32768 + j
    never expects hypothesis j's score or support."""
    c = launch_split_case()
    P = c["P"]
    idx = seam_index(P, 8)
    poses = c["poses"][idx]
    sup8, n = supports_of(c["renders"], c["scene"], c["tau"])
    sup = [sup8[idx[i]] for i in range(P)]
    order = np.arange(P)[::-1] if reverse else np.arange(P)
    want = cover_ref(sup, n, order, 1, 4, 1, KEEP_ALL)
    sc, cov, frame, sel = api.score_cover(c["tris"], poses, c["W"], c["H"], c["proj"], c["scene"], c["tau"], order, (1, 4), 1, None)
    assert_seam_visible(c["scores"], idx)
    assert_records_take(sc, c["scores"], idx)
    assert_cover_equal((cov, frame, sel), want)
    assert len(sel) >= 3 and ((np.asarray(sel) >= 32768).any() if reverse else (np.asarray(sel) < 8).all())
    behind = cov["state"][32768:]
    assert (behind != NOT_IN_ORDER).all() and ((behind == ACCEPTED).any() if reverse else (behind != ACCEPTED).all())
