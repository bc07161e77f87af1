"""GPU tests (-m gpu) of the normal agreement: pr_score_normals held to the numpy restatement of the header's definition (tests/normals_ref.py)
over the oracle's renders -- every record byte for byte, int32 and uint16 scenes, with and without ROI, the scores against pr_score_poses, a
frame whose width is no multiple of 64, a batch of several depth chunks and one of two launches over its boxes."""
import numpy as np
import pytest

import oracle_lib as O
from pose_refine_amd import _lib, api, synth
from gpu_common import raw_h2d
from normals_ref import assert_identities, assert_normals_equal, normals_ref
from seam_cases import assert_records_take, assert_seam_visible, seam_index
from verify_ref import assert_scores_equal, launch_split_case, score_ref

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
W, H = 320, 240                                                   # half the scenario's frame: K_TEST / 2
K = np.ascontiguousarray(synth.K_TEST * np.float32(0.5))
K[8] = 1.0
COS30 = float(np.cos(np.deg2rad(30.0)))
TRIPLES = [(10, 20, 0.0), (6, 8, 1.0), (10, 20, COS30)]           # (tau, jump, cos_min)
NOTHING = 27                                                      # the hypothesis behind the camera


@pytest.fixture(scope="module")
def proj():
    return O.compute_proj(K, W, H)


@pytest.fixture(scope="module")
def hyps():
    """28 hypotheses: 20 of the seeded stream (the model pose first), the scene pose pushed over the left, right, top and bottom border and
    into a corner, two far away (narrow boxes), one behind the camera (renders nothing)."""
    base = synth.scene_pose()
    extra = np.stack([base.copy() for _ in range(8)])
    extra[0, 0, 3] -= 175.0
    extra[1, 0, 3] += 170.0
    extra[2, 1, 3] -= 135.0
    extra[3, 1, 3] += 125.0
    extra[4, 0, 3] -= 185.0
    extra[4, 1, 3] += 110.0
    extra[5, 2, 3] = 900.0
    extra[6, :3, 3] = [150.0, -90.0, 1100.0]
    extra[7, 2, 3] = -300.0
    return np.ascontiguousarray(np.concatenate([synth.hypotheses(20), extra]))


@pytest.fixture(scope="module")
def renders(obj06_tris, hyps, proj):
    return O.render(obj06_tris, hyps, W, H, proj)


@pytest.fixture(scope="module")
def scene(obj06_tris, proj):
    """The scene pose's render with holes and +-8 mm noise, as the contour tests make theirs, in front of a slanted wall.  int32, every value in uint16 range."""
    d = O.render(obj06_tris, synth.scene_pose()[None], W, H, proj)[0].astype(np.int64)
    rng = np.random.default_rng(2)
    wall = 360 + np.broadcast_to(np.arange(W), d.shape) // 6
    d = np.where(d > 0, d, wall)
    d = np.where(rng.random(d.shape) < 0.1, 0, d + rng.integers(-8, 9, d.shape))
    return np.ascontiguousarray(d.astype(np.int32))


_REF_CACHE = {}


def _want(renders, scene, step, triple):
    """The reference for the 28 hypotheses (the same for both scene types: the scene's values fit uint16), computed once."""
    key = (step, triple)
    if key not in _REF_CACHE:
        tau, jump, cos_min = triple
        _REF_CACHE[key] = normals_ref(renders, scene, tau, K, step, jump, cos_min)
    return _REF_CACHE[key]


def test_hypotheses_cover_the_box_walk(renders):
    """What the parity test relies on: boxes wider and narrower than a 64-column strip, taller than a 16-row block, across every border, an empty one."""
    drawn = renders > 0
    cols, rows = drawn.any(1).sum(1), drawn.any(2).sum(1)         # (contiguous silhouettes: the counts are the boxes' sides)
    assert (cols > 64).any() and ((cols > 0) & (cols < 64)).any() and (rows > 16).sum() >= 20
    assert drawn[20, :, 0].any() and drawn[21, :, W - 1].any() and drawn[22, 0, :].any() and drawn[23, H - 1, :].any()
    assert drawn[24, :, 0].any() and drawn[24, H - 1, :].any()
    assert not drawn[NOTHING].any() and drawn[:NOTHING].any((1, 2)).all()


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("step", [1, 4, 8])
@pytest.mark.parametrize("triple", TRIPLES)
def test_parity(gpu, model, hyps, proj, scene, renders, triple, step, dtype):
    tau, jump, cos_min = triple
    assert scene.min() >= 0 and scene.max() < 2**16
    sd = api.DeviceVector.from_host(np.ascontiguousarray(scene.astype(dtype)).reshape(-1))
    want = _want(renders, scene, step, triple)
    scores, got = api.score_normals(model, hyps, W, H, proj, sd, tau, K, step, jump, cos_min)
    print(f"step {step} (tau, jump, cos) {triple}: got {[int(got[f].sum()) for f in ('tested', 'agree', 'disagree', 'no_render_normal', 'no_scene_normal')]}")
    assert_normals_equal(got, want)
    assert scores.tobytes() == api.score_poses(model, hyps, W, H, proj, sd, tau).tobytes()
    assert_scores_equal(scores, score_ref(renders, scene, tau))
    assert_identities(got, scores)
    assert got[NOTHING].tobytes() == bytes(32) and scores[NOTHING].tobytes() == bytes(32)
    for f in ("tested", "no_render_normal", "no_scene_normal") + (("agree",) if cos_min < 1.0 else ()) + (("disagree",) if cos_min > 0.0 else ()):
        assert want[f].sum() > 0, f                               # every class occurs, or the test proves little


@pytest.mark.parametrize("roi", [(90, 50, 190, 170), (170, 125, 64, 45)])
def test_roi_parity(gpu, model, obj06_tris, hyps, proj, scene, roi):
    """Two windows inside the frame; the second cuts the silhouettes, so normals within `step` of the window's edge are undefined."""
    poses = hyps[:24]
    r = O.render(obj06_tris, poses, W, H, proj, roi)
    if roi[2] == 64:
        assert (r[:, :, 0] > 0).any() and (r[:, :, -1] > 0).any() and (r[:, 0, :] > 0).any() and (r[:, -1, :] > 0).any()
    for step, (tau, jump, cos_min) in ((4, TRIPLES[2]), (1, TRIPLES[0]), (8, TRIPLES[2])):
        want = normals_ref(r, scene, tau, K, step, jump, cos_min, roi)
        assert want["tested"].sum() > 0 and want["no_render_normal"].sum() > 0
        for dt in (np.int32, np.uint16):
            s = np.ascontiguousarray(scene.astype(dt))
            scores, got = api.score_normals(model, poses, W, H, proj, s, tau, K, step, jump, cos_min, roi=roi)
            assert_normals_equal(got, want)
            assert_scores_equal(scores, score_ref(r, s, tau, roi))
            assert_identities(got, scores)


def test_self_agreement(gpu, model, hyps, proj, renders):
    """A render scored against itself: every tested pixel agrees, at cos_min = 1 too, and the scene has a normal wherever the render has one."""
    for i in (0, 3, 20, 25):
        img = np.ascontiguousarray(renders[i])
        for dt in (np.int32, np.uint16):
            for cos_min in (COS30, 1.0):
                scores, got = api.score_normals(model, hyps[i:i + 1], W, H, proj, np.ascontiguousarray(img.astype(dt)), 0, K, 4, 20, cos_min)
                assert_normals_equal(got, normals_ref(img[None], img, 0, K, 4, 20, cos_min))
                assert got["tested"][0] > 0 and got["agree"][0] == got["tested"][0] and got["disagree"][0] == 0 and got["no_scene_normal"][0] == 0
                assert scores["inlier"][0] == scores["visible"][0] == np.count_nonzero(img)


def test_overlap_from_the_same_render(gpu, model, hyps, proj, scene):
    for dt in (np.int32, np.uint16):
        sd = api.DeviceVector.from_host(np.ascontiguousarray(scene.astype(dt)).reshape(-1))
        scores, nrm, ov = api.score_normals(model, hyps, W, H, proj, sd, 10, K, 4, 20, COS30, want_overlap=True)
        s2, ov2 = api.score_overlap(model, hyps, W, H, proj, sd, 10)
        assert scores.tobytes() == s2.tobytes() and ov.tobytes() == ov2.tobytes() and ov.shape == (len(hyps), len(hyps))
        s3, n3 = api.score_normals(model, hyps, W, H, proj, sd, 10, K, 4, 20, COS30)
        assert s3.tobytes() == scores.tobytes() and n3.tobytes() == nrm.tobytes()
        assert np.array_equal(np.diag(ov), scores["inlier"]) and nrm["tested"].max() > 0


def test_multi_mesh_matches_single_mesh_calls(gpu, obj06_tris, hyps, proj, scene):
    """Two meshes interleaved (and an empty third): every record is what one single-mesh call per mesh gives."""
    meshes = [obj06_tris, np.ascontiguousarray(obj06_tris * np.float32(0.8)), np.zeros((0, 3, 3), np.float32)]
    idx = np.arange(len(hyps)) % 2
    idx[5] = idx[12] = 2
    for dt in (np.int32, np.uint16):
        sd = api.DeviceVector.from_host(np.ascontiguousarray(scene.astype(dt)).reshape(-1))
        sc, nrm, ov = api.score_normals_multi(meshes, idx, hyps, W, H, proj, sd, 10, K, 4, 20, COS30, want_overlap=True)
        want_sc, want_n = np.zeros(len(hyps), api.SCORE), np.zeros(len(hyps), api.NORMAL)
        for m in range(3):
            sel = np.flatnonzero(idx == m)
            want_sc[sel], want_n[sel] = api.score_normals(meshes[m], hyps[sel], W, H, proj, sd, 10, K, 4, 20, COS30)
        assert sc.tobytes() == want_sc.tobytes() and nrm.tobytes() == want_n.tobytes()
        s2, ov2 = api.score_overlap_multi(meshes, idx, hyps, W, H, proj, sd, 10)
        assert s2.tobytes() == sc.tobytes() and ov2.tobytes() == ov.tobytes()
        assert (nrm["tested"][idx == 2] == 0).all() and (nrm["tested"][idx == 0][:8] > 0).all() and nrm["tested"][idx == 1].sum() > 0


def test_scene_is_read_on_every_call(gpu, model, hyps, proj, scene, renders):
    poses, r = hyps[:16], renders[:16]
    other = np.ascontiguousarray(np.where(scene > 0, scene + 3, 0)[::-1, ::-1])
    for dt in (np.int32, np.uint16):
        s1, s2 = np.ascontiguousarray(scene.astype(dt)), np.ascontiguousarray(other.astype(dt))
        sd = api.DeviceVector.from_host(s1.reshape(-1))
        first = api.score_normals(model, poses, W, H, proj, sd, 10, K, 4, 20, COS30)[1]
        assert_normals_equal(first, normals_ref(r, s1, 10, K, 4, 20, COS30))
        raw_h2d(sd.data(), s2)                                    # the frame rewritten behind the library's back
        second = api.score_normals(model, poses, W, H, proj, sd, 10, K, 4, 20, COS30)[1]
        assert_normals_equal(second, normals_ref(r, s2, 10, K, 4, 20, COS30))
        assert first.tobytes() != second.tobytes()


def test_int32_extremes(gpu, obj06_tris):
    """Depths near INT32_MAX beside depths of 1 on a small frame: the differences need 64 bits, the normals double -- no overflow, parity holds."""
    w, h = 96, 72
    k = np.ascontiguousarray(synth.K_TEST * np.float32(0.15))
    pj = O.compute_proj(k, w, h)
    tris = obj06_tris
    poses = synth.hypotheses(8)
    r = O.render(tris, poses, w, h, pj)
    assert (r > 0).any((1, 2)).all()
    rng = np.random.default_rng(8)
    vals = np.array([INT32_MAX, INT32_MAX - 1, INT32_MAX - 1000, 1, 2, 300, 310, 0, -1, -INT32_MAX - 1], np.int64)
    ext = np.repeat(np.repeat(rng.choice(vals, size=(h // 3, w // 3)), 3, 0), 3, 1).astype(np.int32)
    seen = set()
    for tau, step, jump, cos_min in ((INT32_MAX, 1, 0, COS30), (INT32_MAX, 1, 1000, 0.0), (INT32_MAX, 3, INT32_MAX, COS30), (INT32_MAX, 2, INT32_MAX - 2, 1.0),
                                     (1000, 1, INT32_MAX, COS30)):
        scores, got = api.score_normals(tris, poses, w, h, pj, ext, tau, k, step, jump, cos_min)
        want = normals_ref(r, ext, tau, k, step, jump, cos_min)
        assert_normals_equal(got, want)
        assert_scores_equal(scores, score_ref(r, ext, tau))
        assert_identities(got, scores)
        seen.add((int(got["tested"].sum()), int(got["agree"].sum())))
    assert len(seen) >= 4 and max(t for t, _ in seen) > 0


def test_edge_cases_and_argument_errors(gpu, model, hyps, proj, scene):
    lib = _lib.load()
    pj = np.ascontiguousarray(proj, np.float32)
    sd = api.DeviceVector.from_host(scene.reshape(-1))
    no_roi = _lib.Roi(0, 0, 0, 0)
    # no hypotheses: PR_OK, nothing written (null pointers allowed)
    assert lib.pr_score_normals(None, 0, None, 0, W, H, pj.ctypes.data, no_roi, None, 1, 5, None, 4, 20, 0.5, None, None, None) == _lib.PR_OK
    sc, nrm = api.score_normals(model, np.zeros((0, 4, 4), np.float32), W, H, pj, sd, 5, K, 4, 20, 0.5)
    assert len(sc) == 0 and len(nrm) == 0
    sc, nrm = api.score_normals_multi([model], np.zeros(0, np.int64), np.zeros((0, 4, 4), np.float32), W, H, pj, sd, 5, K, 4, 20, 0.5)
    assert len(sc) == 0 and len(nrm) == 0
    # an empty mesh renders nothing
    nrm = api.score_normals(api.Model(tris=np.zeros((0, 3, 3), np.float32)), hyps[:5], W, H, pj, sd, 5, K, 4, 20, 0.5)[1]
    assert nrm.tobytes() == bytes(32 * 5)
    # refused calls leave the output arrays untouched
    poses = np.ascontiguousarray(hyps[:16], np.float32)
    td = model.device_tris()
    sc, nrm = np.full(16 * 32, 7, np.uint8).view(api.SCORE), np.full(16 * 32, 7, np.uint8).view(api.NORMAL)
    before = sc.tobytes(), nrm.tobytes()

    def call(tau=5, k_p=K.ctypes.data, step=4, jump=20, cos_min=0.5, scene_p=sd.data(), sc_p=sc.ctypes.data, n_p=nrm.ctypes.data, roi=no_roi, n=16, ov=None):
        return lib.pr_score_normals(td.data(), td.size() // 9, poses.ctypes.data, n, W, H, pj.ctypes.data, roi, scene_p, 1, tau, k_p, step, jump, cos_min, sc_p, n_p, ov)

    for kw in (dict(tau=-1), dict(step=0), dict(step=9), dict(jump=-1), dict(cos_min=-0.1), dict(cos_min=1.5), dict(cos_min=float("nan")), dict(k_p=None),
               dict(n_p=None), dict(sc_p=None), dict(scene_p=None), dict(roi=_lib.Roi(300, 0, 100, 100)), dict(step=0, n=0)):
        assert call(**kw) == _lib.PR_ERR_INVALID, kw
    table = (_lib.MeshRef * 1)(_lib.MeshRef(td.data(), td.size() // 9))
    idx = np.zeros(16, np.uint32)
    for k_p, step, n_p in ((None, 4, nrm.ctypes.data), (K.ctypes.data, 9, nrm.ctypes.data), (K.ctypes.data, 4, None)):
        assert lib.pr_score_normals_multi(table, 1, idx.ctypes.data, poses.ctypes.data, 16, W, H, pj.ctypes.data, no_roi, sd.data(), 1, 5, k_p, step, 20, 0.5,
                                          sc.ctypes.data, n_p, None) == _lib.PR_ERR_INVALID
    assert (sc.tobytes(), nrm.tobytes()) == before
    assert call() == _lib.PR_OK and (nrm["tested"] > 0).all() and (nrm["reserved"] == 0).all()
    with pytest.raises(api.PoseRefineError) as e:
        api.score_normals(model, hyps[:4], W, H, pj, sd, 5, K, api.NORMAL_MAX_STEP + 1, 20, 0.5)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_score_normals: step" in str(e.value)
    with pytest.raises(api.PoseRefineError) as e:                 # the message names the entry point that was called
        api.score_normals_multi([model], np.zeros(4, np.int64), hyps[:4], W, H, pj, sd, -1, K, 4, 20, 0.5)
    assert e.value.code == _lib.PR_ERR_INVALID and "pr_score_normals_multi: tau_mm" in str(e.value)
    with pytest.raises(ValueError):
        api.score_normals(model, hyps[:4], W, H, pj, sd, 5, K[:8], 4, 20, 0.5)


SPLIT_K = np.array([60.0, 0, 23.5, 0, 60.0, 15.5, 0, 0, 1], np.float32)      # the intrinsics launch_split_case's projection is made from


@pytest.mark.parametrize("dtype", [np.int32, np.uint16])
@pytest.mark.parametrize("step", [1, 8])
def test_parity_on_a_frame_narrower_than_a_strip(gpu, step, dtype):
    """The 48 x 32 frame of verify_ref.launch_split_case: a width that is no multiple of 64, renders that reach all four borders.  With
    step 8 most neighbours leave the box, and many the frame."""
    c = launch_split_case()
    assert np.array_equal(c["proj"], api.compute_proj(SPLIT_K, c["W"], c["H"]))
    scene = np.ascontiguousarray(c["scene"].astype(dtype))
    want = normals_ref(c["renders"], c["scene"], c["tau"], SPLIT_K, step, c["jump"], COS30)
    scores, got = api.score_normals(c["tris"], c["poses"], c["W"], c["H"], c["proj"], scene, c["tau"], SPLIT_K, step, c["jump"], COS30)
    assert_normals_equal(got, want)
    assert_scores_equal(scores, c["scores"])
    assert_identities(got, scores)
    assert want["no_render_normal"].sum() > 0 and (step == 8 or want["tested"].sum() > 0)


def test_chunked_batch_matches_small_batches(gpu, model):
    """The 8192 x 2048 frame of test_verify_gpu.py (2^24 pixels): a chunk of the depth workspace holds 64 hypotheses, so 150 span three chunks."""
    Wb, Hb = 8192, 2048
    Kb = np.array([1200.0, 0, Wb / 2, 0, 1200.0, Hb / 2, 0, 0, 1], np.float32)
    pj = api.compute_proj(Kb, Wb, Hb)
    poses = synth.hypotheses(150, seed=9)
    sc = api.render_host(model, synth.scene_pose()[None], Wb, Hb, pj)[0]
    rng = np.random.default_rng(2)
    sc = np.where(rng.random(sc.shape) < 0.1, 0, sc + rng.integers(-8, 9, sc.shape) * (sc > 0)).astype(np.int32)
    sd = api.DeviceVector.from_host(sc.reshape(-1))
    whole = api.score_normals(model, poses, Wb, Hb, pj, sd, 4, Kb, 2, 20, COS30)
    parts = [api.score_normals(model, poses[i:i + 40], Wb, Hb, pj, sd, 4, Kb, 2, 20, COS30) for i in range(0, 150, 40)]
    assert_scores_equal(whole[0], np.concatenate([p[0] for p in parts]))
    assert_normals_equal(whole[1], np.concatenate([p[1] for p in parts]))
    assert whole[0].tobytes() == api.score_poses(model, poses, Wb, Hb, pj, sd, 4).tobytes()
    assert_identities(whole[1], whole[0])
    assert (whole[0]["visible"] > 0).all() and (whole[1]["tested"][64:] > 0).any() and (whole[1]["tested"][128:] > 0).any()


def test_batch_of_two_box_launches(gpu):
    """32768 + 5 hypotheses in one depth chunk: the launches over their boxes are split in two (grid.y is limited), and the second starts at
    its own records.  Every score and normal record is the reference's for its pose, the ones behind the split included; uint16 scene.
    Behind the split every hypothesis takes the next pose (seam_cases.seam_index), so hypothesis 32768 + j never expects hypothesis j's records."""
    c = launch_split_case()
    idx = seam_index(c["P"], 8)
    poses = c["poses"][idx]
    scene = np.ascontiguousarray(c["scene"].astype(np.uint16))
    want = normals_ref(c["renders"], c["scene"], c["tau"], SPLIT_K, 1, c["jump"], COS30)
    assert want["tested"].sum() > 0 and len(set(want["tested"].tolist())) > 4      # records that tell the poses apart
    assert_seam_visible(want, idx)
    scores, got = api.score_normals(c["tris"], poses, c["W"], c["H"], c["proj"], scene, c["tau"], SPLIT_K, 1, c["jump"], COS30)
    assert_records_take(got, want, idx)
    assert_records_take(scores, c["scores"], idx)
