"""The pixel boxes on hard poses, through the host twin (pr_debug_tight_box: pose_box.h compiled for the host, no device), against the
oracle's full-frame raster (tests/oracle_lib.py), which knows no boxes: on every hypothesis of tests/box_stress.py's batches, with and
without a ROI that cuts the silhouettes, and on a sweep of a few thousand poses per family, the tight box lies in the loose box, every
drawn pixel lies in both, and the tight box is what the float32 numpy restatement gives.  What the device makes of the same batches is
tests/test_box_stress_gpu.py.

The pair kernels (VSD, interpenetration, overlap), the contour fit and the information pass are held to the same renders there; here their
references are pinned on the hard poses -- the near plane of solid_ref.span_ref is the oracle's render, negative depths included -- and
`assert_pair_classes` states what the batches must contain for those tests to mean anything."""
import numpy as np
import pytest

import oracle_lib as O
from box_stress import (FIT_TJR, H, NONE, ROIS, W, assert_boxes_hold, assert_classes, assert_pair_classes, batch_boxes, drawn_count, one_truths, pair_records,
                        returned_planes, roi_renders, span_planes, stress_batches, sweep_groups)
from solid_ref import INT_MAX, check_invariants, span_ref


def test_the_batches_hold_every_class():
    print(assert_classes(stress_batches()))


@pytest.mark.parametrize("roi", [NONE] + ROIS)
def test_boxes_of_the_batches_hold_every_drawn_pixel(roi):
    cut = 0
    for k, b in enumerate(stress_batches()):
        R = b["R"] if roi == NONE else roi_renders(k, roi)
        if roi != NONE:
            full = b["R"][:, roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]
            assert np.array_equal(R, full), b["name"]               # (the oracle's window is the window of its frame)
            cut += int(((R[:, :, 0] > 0).any(1) | (R[:, :, -1] > 0).any(1) | (R[:, 0, :] > 0).any(1) | (R[:, -1, :] > 0).any(1)).sum())
        for i, pose in enumerate(b["poses"]):
            assert_boxes_hold(b["tris"], pose, b["proj"], R[i], roi, what=(b["name"], i, b["families"][i]))
    assert roi == NONE or cut >= 50                               # the window does cut silhouettes


def test_boxes_hold_on_a_sweep_of_every_family():
    n = drawn = 0
    for name, tris, K, poses in sweep_groups():
        poses = np.ascontiguousarray(poses, np.float32)
        proj = O.compute_proj(K, W, H)
        R = O.render(tris, poses, W, H, proj)
        for i, pose in enumerate(poses):
            drawn += assert_boxes_hold(tris, pose, proj, R[i], what=(name, i))[2] is not None
        n += len(poses)
    print(f"{n} poses, {drawn} of them draw something")
    assert n >= 15000 and 2 * drawn >= n


# ---- the references of the pair kernels and the contour fit on the same batches -----------------------------------------------------------
def test_near_plane_of_the_span_reference_is_the_oracles_render():
    """On every batch, the hypotheses with fragments behind the camera included: the minimum composite of solid_ref's fragments, INT_MAX
    mapped to 0, is R bit for bit; the far plane is never in front of it and is drawn exactly where the near plane is."""
    behind = 0
    for k, b in enumerate(stress_batches()):
        near, far = span_planes(k)
        drawn = near != INT_MAX
        assert np.array_equal(np.where(drawn, near, 0), b["R"]), b["name"]
        assert np.array_equal(returned_planes(k)[0], b["R"]), b["name"]
        assert np.array_equal(far != np.iinfo(np.int32).min, drawn) and (far[drawn] >= near[drawn]).all(), b["name"]
        behind += int((near < 0).any((1, 2)).sum())
        check_invariants(pair_records(k, 0))
    assert behind >= 4
    b = stress_batches()[0]                                       # (the cached planes are span_ref's, and its raw=False form is returned_planes)
    some = [i for i, f in enumerate(b["families"]) if f == "straddle"]
    near, far = span_ref(b["tris"], b["poses"][some], b["proj"], W, H)
    assert np.array_equal(near, returned_planes(0)[0][some]) and np.array_equal(far, returned_planes(0)[1][some]) and (near < 0).any()


def test_the_batches_hold_every_pair_class():
    print(FIT_TJR, assert_pair_classes(stress_batches()))


def test_one_truths_are_a_whole_frame_and_nothing():
    for k, b in enumerate(stress_batches()[:2]):
        whole, nothing = one_truths(k)
        n = drawn_count(b["R"])
        assert b["families"][whole] == "close" and batch_boxes(k)[0][whole].tolist() == [0, 0, W - 1, H - 1] and n[whole] > 2000, (b["name"], n[whole])
        assert b["families"][nothing] == "nothing" and n[nothing] == 0, (b["name"], n[nothing])
