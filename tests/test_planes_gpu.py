"""Support planes on the device: pr_scene_planes_dev against the numpy reference (tests/planes_ref.py) and the host twin, byte for byte -- the
support table of every round, the winner, the ten moments, labelled / behind, the label image and the cleared depth -- and the table scenario."""
import ctypes as C
import math

import numpy as np
import pytest

import planes_cases as PC
import planes_ref as R
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
F = np.float32


def dev_scene(pcd, nrm, w, h, K=synth.K_TEST):
    sc = api.Scene_projective()
    sc.width, sc.height, sc.K = w, h, np.asarray(K, F)
    sc.pcd_buffer = api.DeviceVector.from_host(np.ascontiguousarray(pcd, F).reshape(-1))
    sc.normal_buffer = api.DeviceVector.from_host(np.ascontiguousarray(nrm, F).reshape(-1))
    return sc


def run_dev(sc, depth, pkw, **extra):
    planes, labels, cleared, moments, supports = api.scene_planes(sc, depth, want_moments=True, want_supports=True, **pkw, **extra)
    return planes, labels.to_host().reshape(sc.height, sc.width), cleared.to_host().reshape(sc.height, sc.width), moments, supports


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def synthetic_refs(gpu):
    """the reference once per frame family (the host test's variants: the three strides, samples exactly at r == tau and dot == cos_min, a tie,
    one candidate, the normal test off, a peel that ends early, drop_behind both ways; holes, depth without a normal, z <= 0 and z beyond 65 535 mm
    in every frame; sample and candidate counts that are no multiple of 256 or 64)"""
    out = {}
    for name, fkw, pkw in PC.synthetic_variants():
        pcd, nrm, depth, _ = PC.synthetic(**fkw)
        out[name] = (dev_scene(pcd, nrm, PC.W, PC.H), pcd, nrm, depth, pkw, R.scene_planes(pcd, nrm, depth, PC.W, PC.H, **pkw))
    return out


@pytest.mark.parametrize("name", [v[0] for v in PC.synthetic_variants()])
@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_device_equals_reference_and_host(synthetic_refs, name, dtype):
    sc, pcd, nrm, depth, pkw, ref = synthetic_refs[name]
    assert ref["n_samples"] % 256 != 0 and (ref["n_candidates"] % 64 != 0 or ref["n_candidates"] == 1)
    ref = dict(ref, depth=ref["depth"].astype(dtype))
    got = run_dev(sc, depth.astype(dtype), pkw)
    PC.assert_same(got, ref, pkw["n_planes"])
    assert same_bytes(run_dev(sc, depth.astype(dtype), pkw), got)                     # the same call twice
    host = api.scene_planes_host(pcd, nrm, depth.astype(dtype), PC.W, PC.H, want_moments=True, want_supports=True, **pkw)
    assert same_bytes(host, got)
    if name == "stride1_edges":
        assert len(got[0]) == 2 and pkw["n_planes"] == 3           # two planted planes, three asked for


def test_depth_out_may_be_the_input_and_none(gpu, synthetic_refs):
    sc, pcd, nrm, depth, pkw, ref = synthetic_refs["stride3"]
    d = api.DeviceVector.from_host(depth.reshape(-1))
    planes, labels, cleared = api.scene_planes(sc, d, depth_out=d, **pkw)
    assert cleared is d and d.to_host().tobytes() == ref["depth"].tobytes() and labels.to_host().tobytes() == ref["labels"].tobytes()
    # no cleared depth wanted: the C entry point takes NULL
    pp = api.PlaneParams(**pkw)
    desc = sc.desc()
    lab = api.DeviceVector(PC.W * PC.H, np.uint8)
    out = np.zeros(_lib.PLANE_MAX_PLANES, _lib.PLANE)
    n = C.c_uint32(0)
    _lib.check(_lib.load().pr_scene_planes_dev(C.addressof(desc), None, 0, C.addressof(pp), lab.data(), None, _lib.ptr(out), None, None, C.byref(n)))
    assert n.value == len(ref["planes"]) and lab.to_host().tobytes() == ref["labels"].tobytes()


def test_wide_frame_several_tiles_per_row(gpu):
    """320 x 240 at stride 2: more sample tiles than the launch has rows for its 15 candidate columns, so a workgroup row walks two tiles and the
    last row is short; about 3 600 candidates (no multiple of 256); two rounds."""
    w, h = 320, 240
    pcd, nrm, depth, facts = PC.synthetic(w, h, seed=21, holes=0.03, bare=0.02)
    pkw = dict(stride=2, cand_stride=5, tau_mm=facts["tau_edge"], label_tau_mm=facts["tau_edge"], cos_min=facts["cos_edge"], min_support=40, n_planes=2, drop_behind=False)
    ref = R.scene_planes(pcd, nrm, depth, w, h, **pkw)
    assert ref["n_samples"] > 69 * 256 and ref["n_samples"] % 256 != 0 and ref["n_candidates"] % 256 != 0 and len(ref["planes"]) == 2
    got = run_dev(dev_scene(pcd, nrm, w, h), depth, pkw)
    PC.assert_same(got, ref, 2)


def test_empty_sample_and_caps(gpu):
    pcd, nrm, depth, _ = PC.synthetic()
    sc = dev_scene(pcd, np.zeros_like(nrm), PC.W, PC.H)
    planes, labels, cleared = api.scene_planes(sc, depth, stride=1, min_support=3)
    lab = labels.to_host().reshape(PC.H, PC.W)
    assert len(planes) == 0 and np.array_equal(lab == 0, pcd[..., 2] > 0) and np.array_equal(lab == api.PLANE_NO_DEPTH, pcd[..., 2] <= 0)
    assert cleared.to_host().tobytes() == depth.tobytes()
    w, h = 320, 240                                                 # 76 800 samples at stride 1: over PLANE_MAX_SAMPLES
    big = dev_scene(np.ones((h, w, 3), F), np.ones((h, w, 3), F), w, h)
    for kw in (dict(stride=1), dict(stride=2, cand_stride=1)):      # ... and 19 200 candidates: over PLANE_MAX_CANDIDATES
        with pytest.raises(api.PoseRefineError) as e:
            api.scene_planes(big, np.ones((h, w), np.uint16), **kw)
        assert e.value.code == _lib.PR_ERR_INVALID


# ---- the scenario: obj_06 on a table -----------------------------------------------------------------------------------------------------------
TABLE_TILT_DEG = 25.0
E2E_N = 2        # twice the rank (1) at which tests/ppf_ref.py alone puts the first hypothesis with ADD < 0.1 d on the cleared frame (profiles/planes/README.md)
OBJECT_SHARE_REF = 0.0      # the share of object pixels tests/planes_ref.py labels as plane on this frame (0 of 21 960: the nearest object pixel is 6.97 mm off the table)


def table_frame(render):
    """(depth uint16, object mask, (n, d)): the analytic table behind the render -- the plane z = const turned 25 degrees about the camera's x
    axis, pushed back until it lies 5 mm (rounded up to a whole mm of offset) behind the object pixel nearest to it"""
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    obj = render > 0
    n = PC.tilted(TABLE_TILT_DEG)
    den = PC.rays(W, H, K) @ n
    d = -(math.ceil((render[obj].astype(np.float64) * np.abs(den[obj])).max()) + 5.0)
    zp = PC.plane_depth(W, H, K, n, d)
    assert (zp[obj] > render[obj]).all() and zp.max() < 65535      # the placement: the table lies behind every object pixel
    return np.where(obj, render, np.rint(zp)).astype(np.uint16), obj, (n, d)


def test_scenario_object_on_a_table(gpu, model):
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    render = api.render_host(model, gt[None], W, H, proj)[0]
    depth, obj, (n, d) = table_frame(render)
    full = api.Scene_projective().init_Scene_projective_cuda(depth, K)
    # 1. the state of things without this stage: the full frame has more samples than the voting takes
    with pytest.raises(api.PoseRefineError) as e:
        api.ppf_scene_points(full, 4)
    assert e.value.code == _lib.PR_ERR_INVALID
    # 2. one plane, the analytic one
    depth_dev = api.DeviceVector.from_host(depth.reshape(-1))
    pp = api.PlaneParams()
    planes, labels, cleared = api.scene_planes(full, depth_dev, params=pp)
    assert len(planes) == 1
    lab = labels.to_host().reshape(H, W)
    pmm = full.pcd_host.astype(np.float64) * 1000.0
    pts, nm, pix = R.sample(full.pcd_host, full.normal_host, W, H, pp.stride)              # the winner's inliers: what the plane was fitted to
    inl = R.inliers(pts, nm, np.ones(len(pts), bool), int(planes[0]["candidate"]) * pp.cand_stride, pp.tau_mm, pp.cos_min)
    assert int(inl.sum()) == planes[0]["support"] and not obj.reshape(-1)[pix[inl]].any()  # the bound's premise: samples of the table alone ...
    on = pts[inl].astype(np.float64)
    delta, tan_theta, off_bound = PC.fit_bound(on, n, d, K, W, H)
    assert np.abs(on @ n - d).max() <= delta                                               # ... each within delta of it
    nf = planes[0]["normal"].astype(np.float64)
    cosang = float(nf @ n)
    tan_fit = math.sqrt(max(0.0, 1.0 - cosang * cosang)) / cosang
    print(f"table: support {planes[0]['support']}, labelled {planes[0]['labelled']}, tan(angle) {tan_fit:.3e} (bound {tan_theta:.3e}), "
          f"offset error {abs(float(planes[0]['offset_mm']) - d):.4f} mm (bound {off_bound:.4f})")
    assert cosang > 0 and tan_fit <= tan_theta and abs(float(planes[0]["offset_mm"]) - d) <= off_bound
    assert not (lab[obj] == api.PLANE_BEHIND).any()
    # the cap: the object pixels within a label_tau_mm ring of the contact line -- those the label test could take if the fit were off by its
    # whole bound: analytic distance to the table <= 2 * label_tau_mm.  The reference's figure on this frame is OBJECT_SHARE_REF.
    label_tau = pp.label_tau_mm
    dist = np.abs(pmm @ n - d).reshape(H, W)
    cap = float((dist[obj] <= 2.0 * label_tau).mean())
    share = float((lab[obj] == 1).mean())
    print(f"object pixels labelled as plane: {share:.5f} (reference {OBJECT_SHARE_REF}, cap {cap:.5f})")
    assert OBJECT_SHARE_REF <= cap and share <= cap
    assert (cleared.to_host().reshape(H, W)[obj] == depth[obj])[lab[obj] == 0].all()
    # 3. hypotheses from the cleared frame, at the defaults
    scene = api.Scene_projective().init_Scene_projective_device(cleared, K, W, H)
    pm = api.PPFModel(model)
    hyp, votes = api.generate_hypotheses(pm, scene)
    v64 = model.vertices.astype(np.float64)
    sq = (v64 * v64).sum(1)
    diam = math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))
    add = api.mean_displacement(api.pose_distance(model, hyp, gt))
    first = int(np.flatnonzero(add < 0.1 * diam)[0]) + 1 if (add < 0.1 * diam).any() else None
    print(f"cleared frame: {len(hyp)} hypotheses, first with ADD < 0.1 d at rank {first}; ADD of the first {E2E_N}: {add[:E2E_N]}")
    assert (add[:E2E_N] < 0.1 * diam).any()
