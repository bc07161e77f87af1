"""pr_ppf_vote_multi on the device: a table of point-pair-feature models over one scene sample in one call.  Every model's slice is held to the
single call (pr_ppf_vote) byte for byte and, for two of the models, to the numpy restatement (tests/ppf_ref.py); then a frame with two objects end
to end -- hypotheses of both meshes from one vote call, refined as one mixed batch, against the truth."""
import math

import numpy as np
import pytest

import ppf_ref as R
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


# ---- the blob recipe of tests/test_ppf_gpu.py, restated ---------------------------------------------------------------------------------------
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


# ---- small shapes: the table [B, C, A, E, A] over one scene ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_case(gpu):
    """Models A (about 200 points x 30 alpha bins: a cell count that is no multiple of 64), B (512 x 64 = 32768 cells: the whole LDS accumulator),
    C (3 points x 2 alpha bins, n_angle 7: 6 cells, fewer than a wavefront) and E (one point: no pairs, no table entries); the scene of A (498
    points) for all of them; the reference's accumulators of A and C for the 8 references, computed once."""
    A = _ppf_model(13.5, n_alpha=30)
    B = _ppf_model(6.5, 512, n_alpha=64)
    Cm = _ppf_model(13.5, 3, n_angle=7, n_alpha=2)
    E = _ppf_model(13.5, 1)
    assert 150 <= len(A.points) <= 260 and (len(A.points) * 30) % 64 != 0
    assert len(B.points) * B.params.n_alpha == _lib.PPF_MAX_CELLS and len(Cm.points) * Cm.params.n_alpha == 6 and len(E.points) == 1
    sp, sn = _vote_scene(A)
    refs = list(range(0, 498, 71))
    want = {}
    for name, pm in (("A", A), ("C", Cm)):
        tb = R.tables(pm.params)
        offsets, ent = R.model_table(tb, pm.points, pm.normals)
        accs = [R.accumulator(tb, offsets, ent, len(pm.points), sp, sn, r) for r in refs]
        want[name] = dict(tb=tb, acc=np.stack([a for a, _ in accs]), n_pairs=[p for _, p in accs])
    assert want["A"]["acc"].sum() > 0 and want["C"]["acc"].sum() > 0          # (C's three points do collect votes: the check below is not vacuous)
    return dict(models=[B, Cm, A, E, A], names=["B", "C", "A", "E", "A"], sp=sp, sn=sn, refs=refs, want=want,
                dsp=api.DeviceVector.from_host(sp.reshape(-1)), dsn=api.DeviceVector.from_host(sn.reshape(-1)))


@pytest.fixture(params=[0, 1], ids=["lane_walk", "wave_walk"])
def walk(request, gpu):
    """Both bucket walks (option "ppf_walk"); the library's default afterwards."""
    api.set_option("ppf_walk", request.param)
    yield request.param
    api.set_option("ppf_walk", 1)


@pytest.mark.parametrize("n_peaks", [1, 4])
def test_table_equals_single_calls_and_reference(table_case, walk, n_peaks):
    """"E's peaks are all zero" is read as the header states it for a model without pairs: no peak -- votes, model_ref and alpha_bin 0 and an all-zero
    pose in every slot; scene_ref and n_pairs are the reference's own, as in the single call, to which every byte of the slice is held."""
    assert api.get_option("ppf_walk") == walk
    c = table_case
    models, dsp, dsn = c["models"], c["dsp"], c["dsn"]
    peaks, poses, accs = api.ppf_vote_multi(models, dsp, dsn, 498, 0, 71, 8, n_peaks, want_acc=True)
    assert peaks.shape == (5, 8, n_peaks) and poses.shape == (5, 8, n_peaks, 4, 4) and len(accs) == 5
    # 1. every model's slice equals the single call, as bytes
    for k, pm in enumerate(models):
        p1, q1, a1 = api.ppf_vote(pm, dsp, dsn, 498, 0, 71, 8, n_peaks, want_acc=True)
        assert accs[k].dtype == np.uint32 and accs[k].shape == a1.shape == (8, len(pm.points), pm.params.n_alpha)
        assert peaks[k].tobytes() == p1.tobytes() and poses[k].tobytes() == q1.tobytes() and accs[k].tobytes() == a1.tobytes(), c["names"][k]
    # 2. A and C against the reference: accumulators as integers, peaks in the header's order
    for k, name in ((2, "A"), (1, "C")):
        w, pm = c["want"][name], models[k]
        assert np.array_equal(accs[k].astype(np.int64), w["acc"])
        for j, ref in enumerate(c["refs"]):
            want = R.peaks(w["acc"][j], n_peaks)
            for p in range(n_peaks):
                pk = peaks[k, j, p]
                assert pk["scene_ref"] == ref and pk["n_pairs"] == w["n_pairs"][j]
                if p < len(want):
                    assert (int(pk["votes"]), int(pk["model_ref"]), int(pk["alpha_bin"])) == want[p]
                    ref_pose = R.peak_pose(w["tb"], pm.points[want[p][1]], pm.normals[want[p][1]], c["sp"][ref], c["sn"][ref], want[p][2])
                    assert poses[k, j, p].tobytes() == ref_pose.tobytes()
                else:
                    assert pk["votes"] == 0 and pk["model_ref"] == 0 and pk["alpha_bin"] == 0 and not poses[k, j, p].any()
    # 3. the same model twice: the same bytes twice
    assert peaks[2].tobytes() == peaks[4].tobytes() and poses[2].tobytes() == poses[4].tobytes() and accs[2].tobytes() == accs[4].tobytes()
    # 4. the model of one point has no peak
    assert not peaks[3]["votes"].any() and not peaks[3]["model_ref"].any() and not peaks[3]["alpha_bin"].any() and not poses[3].any() and not accs[3].any()
    # 5. a second call gives the same bytes
    peaks2, poses2, accs2 = api.ppf_vote_multi(models, dsp, dsn, 498, 0, 71, 8, n_peaks, want_acc=True)
    assert peaks2.tobytes() == peaks.tobytes() and poses2.tobytes() == poses.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(accs, accs2))
    # 6. a window of the references, no accumulator wanted
    p3, q3 = api.ppf_vote_multi(models, dsp, dsn, 498, 71, 71, 3, n_peaks)
    assert p3.tobytes() == np.ascontiguousarray(peaks[:, 1:4]).tobytes() and q3.tobytes() == np.ascontiguousarray(poses[:, 1:4]).tobytes()
    # 7. a table of one model
    for k in (0, 2):
        p1, q1 = api.ppf_vote(models[k], dsp, dsn, 498, 0, 71, 8, n_peaks)
        p4, q4 = api.ppf_vote_multi([models[k]], dsp, dsn, 498, 0, 71, 8, n_peaks)
        assert p4[0].tobytes() == p1.tobytes() and q4[0].tobytes() == q1.tobytes()


# ---- a frame with two objects, from the frame alone -------------------------------------------------------------------------------------------
E2E_N = 2        # twice the rank (1 for obj_06, 1 for the blob) at which tests/ppf_ref.py alone puts the first hypothesis with ADD < 0.1 d of each mesh in this frame (profiles/ppf_multi/README.md)


def _e2e_blob():
    """The blob of the frame: a finer UV sphere with bumps (768 triangles), stretched differently along every axis (x 1, y 0.7, z 0.45: no two
    axes alike, so a pose that swaps or flips axes has a large ADD), and its pose: left of and above obj_06 in the image, no pixel shared."""
    tris = (synth.uv_sphere_mesh(24, 16).astype(np.float64) * [1.0, 0.7, 0.45]).astype(np.float32)
    q, _ = np.linalg.qr(np.random.default_rng(21).normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return tris, synth.pose_matrix(q.astype(np.float32), np.array([-150.0, -50.0, 400.0], np.float32))


def _diameter(v):
    v64 = np.asarray(v, np.float64)
    sq = (v64 * v64).sum(1)
    return math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))      # the largest vertex distance


def test_two_objects_end_to_end(gpu, model, scenario, obj06_tris):
    """obj_06 at synth.scene_pose() and the blob, the oracle's renders composed (per pixel the nearer non-zero depth) as the frame, default
    parameters: generate_hypotheses_multi equals the two generate_hypotheses calls byte for byte; for each mesh one of the first E2E_N hypotheses
    has ADD < 0.1 d before refinement, and after refine_batch_multi (20 iterations, kd-tree scene) the hypothesis ICP itself rates best per mesh
    (fitness, then rmse) has MSSD < 1 mm."""
    import oracle_lib as O
    W, H, K, proj = synth.WIDTH, synth.HEIGHT, scenario["K"], scenario["proj"]
    blob_tris, blob_pose = _e2e_blob()
    blob = api.Model(tris=blob_tris)
    d_obj = scenario["depth"][1]
    d_blob = O.render(blob_tris, blob_pose[None], W, H, proj)[0]
    assert (d_obj > 0).any() and (d_blob > 0).any() and not ((d_obj > 0) & (d_blob > 0)).any()              # two objects, no pixel shared
    depth = np.where((d_obj > 0) & ((d_blob == 0) | (d_obj < d_blob)), d_obj, d_blob).astype(np.int32)
    scene = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    scene_nn = api.Scene_nn().init_Scene_nn_cuda(depth, K)
    meshes, truths = [model, blob], [synth.scene_pose(), blob_pose]
    pms = [api.PPFModel(model), api.PPFModel(blob)]
    idx, hyp, votes = api.generate_hypotheses_multi(pms, scene)
    assert idx.dtype == np.int32 and hyp.dtype == np.float32 and votes.dtype == np.int64 and np.all(np.diff(idx) >= 0)
    for k, pm in enumerate(pms):
        h1, v1 = api.generate_hypotheses(pm, scene)
        s = idx == k
        assert 0 < len(h1) <= 256 and np.all(np.diff(v1) <= 0)
        assert hyp[s].tobytes() == h1.tobytes() and votes[s].tobytes() == v1.tobytes()
    res, _ = api.refine_batch_multi(meshes, idx, hyp, W, H, proj, K, scene_nn, api.ICPConvergenceCriteria(0.0, 0.0, 20))
    refined = api.refined_poses(res, hyp)
    for k, (mesh, gt) in enumerate(zip(meshes, truths)):
        s = np.flatnonzero(idx == k)
        diam = _diameter(mesh.vertices)
        add = api.mean_displacement(api.pose_distance(mesh, hyp[s], gt))
        first = int(np.flatnonzero(add < 0.1 * diam)[0]) + 1 if (add < 0.1 * diam).any() else None
        print(f"mesh {k}: hypotheses {len(s)}, diameter {diam:.3f}, first with ADD < 0.1 d at rank {first}, {int((add < 0.1 * diam).sum())} such before refinement; ADD of the first {E2E_N}: {add[:E2E_N]}")
        assert (add[:E2E_N] < 0.1 * diam).any()
        d = api.pose_distance(mesh, refined[s], gt)
        r = res[s]
        best = int(np.lexsort((r["inlier_rmse"], -r["fitness"]))[0])
        mssd = api.max_displacement(d)
        print(f"mesh {k}: after refine_batch_multi: {int((api.mean_displacement(d) < 0.1 * diam).sum())} of {len(s)} with ADD < 0.1 d; best by fitness: hypothesis {best}, fitness {r['fitness'][best]:.4f}, MSSD {mssd[best]:.4f} mm")
        assert mssd[best] < 1.0
