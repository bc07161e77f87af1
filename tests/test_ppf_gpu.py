"""Point-pair-feature voting on the device against the numpy restatement (tests/ppf_ref.py): the model's pair table, the scene sample, the
accumulators bit for bit, peaks and poses, and the committed scenario end to end -- hypotheses from the frame alone, refined, against the truth."""
import math

import numpy as np
import pytest

import ppf_ref as R
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


def _blob_tris():
    """A small closed mesh without symmetry: a coarse UV sphere with bumps (160 triangles, radius about 60 mm), stretched."""
    return (synth.uv_sphere_mesh(10, 8).astype(np.float64) * [1.0, 0.8, 0.6]).astype(np.float32)


def _ppf_model(step_mm, n_model=None, **kw):
    """The blob sampled at step_mm (dist_step_mm = step_mm), optionally cut to exactly n_model points (the table is built on first use)."""
    pm = api.PPFModel(_blob_tris(), step_mm=25.0, dist_step_mm=step_mm, **kw)
    pts, nrm = api.ppf_model_sample(_blob_tris(), step_mm)
    assert n_model is None or len(pts) >= n_model
    pm.points, pm.normals, pm.step_mm = np.ascontiguousarray(pts[:n_model]), np.ascontiguousarray(nrm[:n_model]), float(step_mm)
    return pm


# ---- the model's table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_angle", [7, 15])
def test_model_table_equals_reference(gpu, n_angle):
    pm = _ppf_model(13.5, n_angle=n_angle)
    n = len(pm.points)
    assert 150 <= n <= 260 and (n * n) % 256 != 0                  # about 200 points, several workgroups, a ragged last one
    tb = R.tables(pm.params)
    offsets, ent = R.model_table(tb, pm.points, pm.normals)
    d_off, d_ent = pm.table()
    assert pm.n_entries == offsets[-1] > 0
    assert np.array_equal(d_off.astype(np.int64), offsets)         # every bucket's size and place
    key_of = np.repeat(np.arange(tb["n_keys"]), np.diff(offsets))
    o = np.lexsort((d_ent["pair"], key_of))                         # every bucket as a sorted set: the order inside it is not specified
    assert np.array_equal(d_ent["pair"][o], ent["pair"])
    assert np.array_equal(d_ent["cos_m"][o].view(np.uint32), ent["c"].view(np.uint32))      # the float pairs bit for bit
    assert np.array_equal(d_ent["sin_m"][o].view(np.uint32), ent["s"].view(np.uint32))
    again = _ppf_model(13.5, n_angle=n_angle).table()
    assert np.array_equal(again[0], d_off)


# ---- the scene sample -----------------------------------------------------------------------------------------------------------------------
def _synthetic_scene(w=64, h=48, seed=5, blank_row=None):
    rng = np.random.default_rng(seed)
    pcd = rng.uniform(-0.3, 0.3, (h, w, 3)).astype(np.float32)
    pcd[..., 2] = rng.uniform(0.2, 0.9, (h, w)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    hole = rng.random((h, w)) < 0.3
    pcd[hole] = 0                                                   # holes: no depth (and, as the scene preparation leaves them, no normal)
    nrm[hole] = 0
    nrm[rng.random((h, w)) < 0.1] = 0                               # depth without a normal
    pcd[5, 7, 2] = -0.4                                             # a depth that is not > 0
    nrm[0, 0] = [0, 0, -1]; pcd[0, 0] = [0.1, 0.1, 0.5]             # the first pixel kept
    nrm[9, 12] = [0, 1e-30, 0]                                      # one non-zero component is a normal
    pcd[9, 12] = [0.0, 0.0, 0.25]
    if blank_row is not None:
        pcd[blank_row] = 0                                          # a sampled row that keeps nothing
        nrm[blank_row] = 0
    sc = api.Scene_projective()
    sc.width, sc.height, sc.K = w, h, synth.K_TEST
    sc.pcd_buffer = api.DeviceVector.from_host(pcd.reshape(-1))
    sc.normal_buffer = api.DeviceVector.from_host(nrm.reshape(-1))
    return sc, pcd, nrm


# 64 x 48: a row is one 64-column step; 130 x 37: two full steps and a ragged third of two lanes at stride 1, 44 and 33 sampled columns at strides 3
# and 4, a height that neither divides; 70 x 300: 300 row counts, a carry across the scan's 256-chunk.  Row 12 of the two larger frames (sampled at
# every stride) is blank.
@pytest.mark.parametrize("stride", [1, 3, 4])
@pytest.mark.parametrize("w,h", [(64, 48), (130, 37), (70, 300)])
def test_scene_sample_equals_reference(gpu, w, h, stride):
    sc, pcd, nrm = _synthetic_scene(w, h, blank_row=None if (w, h) == (64, 48) else 12)
    want_p, want_n = R.scene_points(pcd, nrm, w, h, stride)
    pts, nr, n = api.ppf_scene_points(sc, stride)
    assert n == len(want_p) > 0
    got_p, got_n = pts.to_host()[:3 * n].reshape(n, 3), nr.to_host()[:3 * n].reshape(n, 3)
    assert got_p.tobytes() == want_p.tobytes() and got_n.tobytes() == want_n.tobytes()
    pts2, nr2, n2 = api.ppf_scene_points(sc, stride)
    assert n2 == n and pts2.to_host()[:3 * n].tobytes() == got_p.tobytes() and nr2.to_host()[:3 * n].tobytes() == got_n.tobytes()


def test_scene_sample_cap(gpu):
    w, h = 160, 120                                                 # 19200 valid pixels: over the cap at stride 1, under it at 2
    sc = api.Scene_projective()
    sc.width, sc.height, sc.K = w, h, synth.K_TEST
    sc.pcd_buffer = api.DeviceVector.from_host(np.ones(w * h * 3, np.float32))
    sc.normal_buffer = api.DeviceVector.from_host(np.ones(w * h * 3, np.float32))
    with pytest.raises(api.PoseRefineError) as e:
        api.ppf_scene_points(sc, 1)
    assert e.value.code == _lib.PR_ERR_INVALID
    assert api.ppf_scene_points(sc, 2)[2] == 80 * 60


# ---- votes, peaks, poses -----------------------------------------------------------------------------------------------------------------------
def _vote_scene(pm, n_scene=498, seed=11):
    """Two moved copies of the model's sample and clutter, n_scene points; references 0, 71, ..., 497 (ref_stride 71): the first and the last
    scene point, one with an axis-aligned normal (71) and one whose neighbours are all beyond the diameter (142)."""
    rng = np.random.default_rng(seed)
    P, N = pm.points.astype(np.float64), pm.normals.astype(np.float64)
    parts_p, parts_n = [], []
    for s in (1, 2):
        q, _ = np.linalg.qr(np.random.default_rng(seed + s).normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        take = rng.permutation(len(P))[:180]
        parts_p.append(P[take] @ q.T + [40.0 * s, -30.0, 300.0 + 25.0 * s]); parts_n.append(N[take] @ q.T)
    m = n_scene - 360
    cn = rng.normal(size=(m, 3))
    parts_p.append(rng.uniform(-80, 80, (m, 3)) + [60, -30, 330]); parts_n.append(cn / np.linalg.norm(cn, axis=1)[:, None])
    sp, sn = np.concatenate(parts_p).astype(np.float32), np.concatenate(parts_n).astype(np.float32)
    o = rng.permutation(n_scene)
    sp, sn = sp[o], sn[o]
    sn[71] = [0.0, 0.0, -1.0]
    sp[142] = sp[0] + np.float32(5.0 * pm.diameter)
    return np.ascontiguousarray(sp), np.ascontiguousarray(sn)


@pytest.fixture(scope="module")
def vote_cases(gpu):
    """(model, scene, the reference's accumulators and pair counts of the 8 references), computed once for: about 200 model points x 30 alpha
    bins (a cell count that is no multiple of 64) and 512 x 64 = 32768 cells exactly (the whole LDS accumulator)."""
    out = {}
    for name, step, kw, n_model in (("ragged", 13.5, dict(n_alpha=30), None), ("full", 6.5, dict(n_alpha=64), 512)):
        pm = _ppf_model(step, n_model, **kw)
        n, na = len(pm.points), pm.params.n_alpha
        if name == "ragged":
            assert (n * na) % 64 != 0
        else:
            assert n * na == _lib.PPF_MAX_CELLS
        tb = R.tables(pm.params)
        sp, sn = _vote_scene(pm)
        offsets, ent = R.model_table(tb, pm.points, pm.normals)
        refs = list(range(0, 498, 71))
        accs = [R.accumulator(tb, offsets, ent, n, sp, sn, r) for r in refs]
        out[name] = dict(pm=pm, tb=tb, sp=sp, sn=sn, refs=refs, acc=np.stack([a for a, _ in accs]), n_pairs=[p for _, p in accs],
                         dsp=api.DeviceVector.from_host(sp.reshape(-1)), dsn=api.DeviceVector.from_host(sn.reshape(-1)))
    return out


@pytest.fixture(params=[0, 1], ids=["lane_walk", "wave_walk"])
def walk(request, gpu):
    """Both bucket walks of pr_ppf_vote (option "ppf_walk"); the library's default afterwards."""
    api.set_option("ppf_walk", request.param)
    yield request.param
    api.set_option("ppf_walk", 1)


@pytest.mark.parametrize("name", ["ragged", "full"])
@pytest.mark.parametrize("n_peaks", [1, 4])
def test_votes_peaks_and_poses_equal_reference(vote_cases, walk, name, n_peaks):
    assert api.get_option("ppf_walk") == walk
    c = vote_cases[name]
    pm, tb = c["pm"], c["tb"]
    peaks, poses, acc = api.ppf_vote(pm, c["dsp"], c["dsn"], 498, 0, 71, 8, n_peaks, want_acc=True)
    assert acc.dtype == np.uint32 and np.array_equal(acc.astype(np.int64), c["acc"])            # every accumulator, bit for bit
    assert c["acc"][2].sum() == 0 and c["n_pairs"][2] == 0 and c["acc"][[0, 1, 7]].sum(axis=(1, 2)).min() > 0
    for j, ref in enumerate(c["refs"]):
        want = R.peaks(c["acc"][j], n_peaks)
        for k in range(n_peaks):
            pk = peaks[j, k]
            assert pk["scene_ref"] == ref and pk["n_pairs"] == c["n_pairs"][j]
            if k < len(want):
                assert (int(pk["votes"]), int(pk["model_ref"]), int(pk["alpha_bin"])) == want[k]
                ref_pose = R.peak_pose(tb, pm.points[want[k][1]], pm.normals[want[k][1]], c["sp"][ref], c["sn"][ref], want[k][2])
                assert poses[j, k].tobytes() == ref_pose.tobytes()                              # the float64 formula, rounded once
            else:                                                                               # an unused slot
                assert pk["votes"] == 0 and pk["model_ref"] == 0 and pk["alpha_bin"] == 0 and not poses[j, k].any()
    assert len(R.peaks(c["acc"][2], n_peaks)) == 0                                              # the lonely reference has no peak
    peaks2, poses2, acc2 = api.ppf_vote(pm, c["dsp"], c["dsn"], 498, 0, 71, 8, n_peaks, want_acc=True)
    assert peaks2.tobytes() == peaks.tobytes() and poses2.tobytes() == poses.tobytes() and acc2.tobytes() == acc.tobytes()
    p3, q3 = api.ppf_vote(pm, c["dsp"], c["dsn"], 498, 71, 71, 3, n_peaks)                      # a window of the references, no accumulator wanted
    assert p3.tobytes() == peaks[1:4].tobytes() and q3.tobytes() == poses[1:4].tobytes()


# ---- the committed scenario, from the frame alone -------------------------------------------------------------------------------------------------
E2E_N = 2        # twice the rank (1) at which tests/ppf_ref.py alone puts the first hypothesis with ADD < 0.1 d for this frame (profiles/ppf/README.md)


def test_scenario_end_to_end(gpu, model, scenario, gscenes):
    """obj_06 at synth.scene_pose(), the oracle's render as the frame, default parameters (stride 4, ref_stride 5): one of the first E2E_N hypotheses
    has ADD < 0.1 d before refinement, and the refined hypothesis ICP itself rates best (fitness, then rmse) has MSSD < 1 mm."""
    W, H, K = synth.WIDTH, synth.HEIGHT, scenario["K"]
    scene = gscenes["proj"]
    pm = api.PPFModel(model)
    tb = R.tables(pm.params)
    # the scene sample and the first 8 references against the reference
    pts, nrm, n_scene = api.ppf_scene_points(scene, 4)
    want_p, want_n = R.scene_points(scene.pcd_host, scene.normal_host, W, H, 4)
    sp, sn = pts.to_host()[:3 * n_scene].reshape(-1, 3), nrm.to_host()[:3 * n_scene].reshape(-1, 3)
    assert n_scene == len(want_p) and sp.tobytes() == want_p.tobytes() and sn.tobytes() == want_n.tobytes()
    offsets, ent = R.model_table(tb, pm.points, pm.normals)
    peaks, poses, acc = api.ppf_vote(pm, pts, nrm, n_scene, 0, 5, 8, 1, want_acc=True)
    for j in range(8):
        a, n_pairs = R.accumulator(tb, offsets, ent, len(pm.points), sp, sn, 5 * j)
        assert np.array_equal(acc[j].astype(np.int64), a) and peaks[j, 0]["n_pairs"] == n_pairs
        (v, m, b), = R.peaks(a, 1)
        assert (int(peaks[j, 0]["votes"]), int(peaks[j, 0]["model_ref"]), int(peaks[j, 0]["alpha_bin"])) == (v, m, b)
        assert poses[j, 0].tobytes() == R.peak_pose(tb, pm.points[m], pm.normals[m], sp[5 * j], sn[5 * j], b).tobytes()
    # hypotheses, refinement, truth
    hyp, votes = api.generate_hypotheses(pm, scene)
    assert 0 < len(hyp) <= 256 and np.all(np.diff(votes) <= 0)
    gt = synth.scene_pose()
    v64 = model.vertices.astype(np.float64)
    sq = (v64 * v64).sum(1)
    diam = math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))      # the largest vertex distance
    add = api.mean_displacement(api.pose_distance(model, hyp, gt))
    first = int(np.flatnonzero(add < 0.1 * diam)[0]) + 1 if (add < 0.1 * diam).any() else None
    print(f"hypotheses {len(hyp)}, first with ADD < 0.1 d at rank {first}, {int((add < 0.1 * diam).sum())} such before refinement; ADD of the first {E2E_N}: {add[:E2E_N]}")
    assert (add[:E2E_N] < 0.1 * diam).any()
    res, _ = api.refine_batch(model, hyp, W, H, scenario["proj"], K, gscenes["nn"], api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = api.refined_poses(res, hyp)
    d = api.pose_distance(model, refined, gt)
    best = int(np.lexsort((res["inlier_rmse"], -res["fitness"]))[0])
    mssd = api.max_displacement(d)
    print(f"after refine_batch: {int((api.mean_displacement(d) < 0.1 * diam).sum())} of {len(hyp)} with ADD < 0.1 d; best by fitness: hypothesis {best}, MSSD {mssd[best]:.4f} mm")
    assert mssd[best] < 1.0
