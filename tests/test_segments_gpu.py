"""Scene segments on the device: pr_scene_segments_dev against the numpy reference (tests/segments_ref.py) and the host twin, byte for byte --
labels, roots, records, counts -- on every case of tests/segments_cases.py and both depth types; pr_segment_depth_dev against numpy; the root cap;
and the scenario of two objects on a table."""
import ctypes as C
import math

import numpy as np
import pytest

import segments_cases as SC
import segments_ref as R
from pose_refine_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


def run_dev(depth, dtype, kw, want_roots=True):
    h, w = depth.shape
    res = api.scene_segments(depth.astype(dtype), w, h, want_roots=want_roots, **kw)
    out = [res[0], res[1].to_host().reshape(h, w)]
    if want_roots:
        out.append(res[2].to_host().reshape(h, w))
    return tuple(out) + (res[-1],)


@pytest.mark.parametrize("name", SC.NAMES)
def test_device_equals_reference_and_host(gpu, name):
    c, ref = SC.BY_NAME[name], SC.reference(name)
    for dtype in c.dtypes:
        what = f"{name} {np.dtype(dtype).name}"
        got = run_dev(c.depth, dtype, c.kw)
        SC.assert_same(got, ref, what)
        again = run_dev(c.depth, dtype, c.kw)                      # the same call twice
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again)), what
        host = api.scene_segments_host(c.depth.astype(dtype), c.depth.shape[1], c.depth.shape[0], want_roots=True, **c.kw)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, host)), what
        bare = run_dev(c.depth, dtype, c.kw, want_roots=False)     # roots_dev_out NULL
        assert bare[0].tobytes() == got[0].tobytes() and bare[1].tobytes() == got[1].tobytes() and bare[-1] == got[-1], what


def test_null_counts(gpu):
    c = SC.BY_NAME["squares_min1"]
    h, w = c.depth.shape
    d = api.DeviceVector.from_host(c.depth.astype(np.uint16).reshape(-1))
    sp = api.SegmentParams(**c.kw)
    lab, seg, n = api.DeviceVector(w * h, np.uint16), np.zeros(sp.max_segments, _lib.SEGMENT), C.c_uint32(0)
    _lib.check(_lib.load().pr_scene_segments_dev(d.data(), 0, w, h, C.addressof(sp), lab.data(), None, _lib.ptr(seg), C.byref(n), None, None))
    ref = SC.reference("squares_min1")
    assert n.value == 7 and seg[:7].tobytes() == ref["segments"].tobytes() and lab.to_host().tobytes() == ref["labels"].tobytes()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_segment_depth_against_numpy(gpu, dtype):
    c, ref = SC.BY_NAME["noise_few_130x77"], SC.reference("noise_few_130x77")
    depth = c.depth.astype(dtype)
    labels = api.DeviceVector.from_host(ref["labels"].reshape(-1))
    for keep in (1, [2], [1, 3, 5], [5, 4, 4], [R.SEGMENT_MAX], []):
        out = api.segment_depth(labels, depth, keep)
        assert out.dtype == depth.dtype and out.to_host().tobytes() == R.segment_depth(ref["labels"], depth, keep).tobytes(), keep
    d = api.DeviceVector.from_host(depth.reshape(-1))              # depth_out may be the input
    assert api.segment_depth(labels, d, [2, 4], depth_out=d) is d
    want = R.segment_depth(ref["labels"], depth, [2, 4])
    assert d.to_host().tobytes() == want.tobytes() and (want != 0).any() and (want[ref["labels"] == R.SEGMENT_DROPPED] == 0).all()
    # a keep table that names label 0 and reaches beyond every label: unmeasured and dropped pixels stay 0
    table = np.ones(R.SEGMENT_MAX + 1, np.uint8)
    out = api.DeviceVector(depth.size, dtype)
    _lib.check(_lib.load().pr_segment_depth_dev(labels.data(), api.DeviceVector.from_host(depth.reshape(-1)).data(), int(dtype == np.int32), depth.size, _lib.ptr(table),
                                                len(table), out.data()))
    assert out.to_host().tobytes() == R.segment_depth(ref["labels"], depth, [1, 2, 3, 4, 5]).tobytes()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_root_cap_refuses_and_leaves_the_outputs(gpu, dtype):
    d = SC.CHECKERBOARD
    h, w = d.shape
    sp = api.SegmentParams(**SC.CHECKERBOARD_KW)
    dep = api.DeviceVector.from_host(d.astype(dtype).reshape(-1))
    labels = api.DeviceVector.from_host(np.full(w * h, 0xABCD, np.uint16))
    roots = api.DeviceVector.from_host(np.full(w * h, 0x12345678, np.uint32))
    segs = np.full(sp.max_segments, 0x5A, np.uint8).repeat(64).view(_lib.SEGMENT)
    n = [C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)]
    rc = _lib.load().pr_scene_segments_dev(dep.data(), int(dtype == np.int32), w, h, C.addressof(sp), labels.data(), roots.data(), _lib.ptr(segs), *[C.byref(v) for v in n])
    assert rc == _lib.PR_ERR_INVALID
    assert (labels.to_host() == 0xABCD).all() and (roots.to_host() == 0x12345678).all() and (segs.view(np.uint8) == 0x5A).all() and [v.value for v in n] == [77, 77, 77]
    # the next call on the same context is not disturbed
    c = SC.BY_NAME["comb_67x45"]
    SC.assert_same(run_dev(c.depth, dtype, c.kw), SC.reference("comb_67x45"))


# ---- the scenario: obj_06 and the blob on a table -----------------------------------------------------------------------------------------------
SCENARIO_JUMP_MM = 20      # at the default 10 tests/segments_ref.py cuts obj_06 in two (shares 0.543 / 1.000); from 15 on each object is one segment (profiles/segments/README.md)
OBJECT_SHARE_REF = {"obj_06": 1.0, "blob": 1.0}      # the share of each mask its largest segment holds: tests/segments_ref.py over scene_planes_host on this frame at SCENARIO_JUMP_MM (21 960 of 21 960, 13 150 of 13 150)
E2E_N = 2        # twice the rank (1) at which tests/ppf_ref.py alone puts the first hypothesis with ADD < 0.1 d on the reference's depth of obj_06's segment (profiles/segments/README.md)


def test_scenario_two_objects_on_a_table(gpu, model):
    """obj_06 at synth.scene_pose() and the bumped blob over the 25-degree table, from the frame alone: scene_planes, then scene_segments on the
    cleared frame (PlaneParams and SegmentParams at their defaults but jump_mm = SCENARIO_JUMP_MM).  No segment lies in both masks, the largest
    segment inside each mask holds the reference's share of it, generate_hypotheses on segment_depth of obj_06's segment finds the pose within
    E2E_N, and the segment's roi scores the true pose as the full frame does."""
    W, H, K = synth.WIDTH, synth.HEIGHT, synth.K_TEST
    proj = api.compute_proj(K, W, H)
    gt = synth.scene_pose()
    blob_tris, blob_pose = SC.blob_mesh_and_pose()
    d_obj = api.render_host(model, gt[None], W, H, proj)[0]
    d_blob = api.render_host(api.Model(tris=blob_tris), blob_pose[None], W, H, proj)[0]
    depth, m_obj, m_blob = SC.two_object_frame(d_obj, d_blob)
    depth_dev = api.DeviceVector.from_host(depth.reshape(-1))
    full = api.Scene_projective().init_Scene_projective_device(depth_dev, K, W, H)
    planes, _, cleared = api.scene_planes(full, depth_dev)
    assert len(planes) == 1
    # 1. the segments of the cleared frame, held to the host twin on the same bytes
    segs, labels, counts = api.scene_segments(cleared, W, H, jump_mm=SCENARIO_JUMP_MM)
    lab = labels.to_host().reshape(H, W)
    hsegs, hlab, hcounts = api.scene_segments_host(cleared.to_host().reshape(H, W), W, H, jump_mm=SCENARIO_JUMP_MM)
    assert segs.tobytes() == hsegs.tobytes() and lab.tobytes() == hlab.tobytes() and counts == hcounts
    in_obj, in_blob = (set(lab[m].tolist()) - {0, R.SEGMENT_DROPPED} for m in (m_obj, m_blob))
    assert not in_obj & in_blob                # no segment has pixels in both masks
    k_obj, share_obj = SC.largest_share(lab, m_obj)
    k_blob, share_blob = SC.largest_share(lab, m_blob)
    print(f"segments {counts}, pixels {segs['pixels'].tolist()}; obj_06: segment {k_obj} holds {share_obj:.5f} of its mask, blob: segment {k_blob} holds {share_blob:.5f}")
    assert k_obj != k_blob and share_obj >= OBJECT_SHARE_REF["obj_06"] and share_blob >= OBJECT_SHARE_REF["blob"]
    # 2. hypotheses from obj_06's segment alone, at the defaults
    kept = api.segment_depth(labels, cleared, k_obj)
    assert kept.to_host().tobytes() == R.segment_depth(lab, cleared.to_host().reshape(H, W), k_obj).tobytes()
    scene = api.Scene_projective().init_Scene_projective_device(kept, K, W, H)
    hyp, votes = api.generate_hypotheses(api.PPFModel(model), scene)
    v64 = model.vertices.astype(np.float64)
    sq = (v64 * v64).sum(1)
    diam = math.sqrt(max(float((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (v64[i:i + 1024] @ v64.T)).max()) for i in range(0, len(v64), 1024)))
    add = api.mean_displacement(api.pose_distance(model, hyp, gt))
    first = int(np.flatnonzero(add < 0.1 * diam)[0]) + 1 if (add < 0.1 * diam).any() else None
    print(f"obj_06's segment: {len(hyp)} hypotheses, first with ADD < 0.1 d at rank {first}; ADD of the first {E2E_N}: {add[:E2E_N]}")
    assert (add[:E2E_N] < 0.1 * diam).any()
    # 3. the segment's box as a roi: it contains the mask, so the true pose scores the same bytes inside it as on the full frame
    seg = segs[k_obj - 1]
    roi = api.segment_roi(seg, W, H)
    ys, xs = np.nonzero(m_obj)
    assert roi[0] <= xs.min() and xs.max() < roi[0] + roi[2] and roi[1] <= ys.min() and ys.max() < roi[1] + roi[3]
    assert roi == R.segment_roi(seg, W, H) and api.segment_roi(seg, W, H, 8) == R.segment_roi(seg, W, H, 8)
    whole = api.score_poses(model, gt[None], W, H, proj, depth_dev, 5)
    boxed = api.score_poses(model, gt[None], W, H, proj, depth_dev, 5, roi=roi)
    assert boxed.tobytes() == whole.tobytes() and int(whole["inlier"][0]) == int(m_obj.sum())
