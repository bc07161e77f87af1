"""The pixel boxes on hard poses, through the host twin (pr_debug_tight_box: pose_box.h compiled for the host, no device), against the
oracle's full-frame raster (tests/oracle_lib.py), which knows no boxes: on every hypothesis of tests/box_stress.py's batches, with and
without a ROI that cuts the silhouettes, and on a sweep of a few thousand poses per family, the tight box lies in the loose box, every
drawn pixel lies in both, and the tight box is what the float32 numpy restatement gives.  What the device makes of the same batches is
tests/test_box_stress_gpu.py."""
import numpy as np
import pytest

import oracle_lib as O
from box_stress import (H, NONE, ROIS, W, assert_boxes_hold, assert_classes, roi_renders, stress_batches, sweep_groups)


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
