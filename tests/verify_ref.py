"""CPU reference of pr_score_poses: a numpy classifier over depth images rendered by the oracle (oracle_lib.render, bit-exact with the
HIP raster).  Integer arithmetic in int64 / Python ints throughout, so the reference itself cannot overflow."""
import functools

import numpy as np

from pose_refine_amd import api, synth

FIELDS = ("visible", "inlier", "occluded", "violation", "missing", "reserved", "abs_err_sum")


def score_ref(renders, scene, tau, roi=(0, 0, 0, 0)):
    """renders: (P, rh, rw) int32 from oracle_lib.render (0 = nothing drawn; with a ROI, the window's pixels);
    scene: (H, W) int32 or uint16 frame.  Returns SCORE[P]."""
    renders = np.asarray(renders)
    scene = np.asarray(scene)
    if roi[2] > 0 and roi[3] > 0:
        x, y, w, h = roi
        scene = scene[y:y + h, x:x + w]
    r = renders.astype(np.int64)
    s = np.broadcast_to(scene.astype(np.int64), r.shape)
    vis = r > 0
    meas = vis & (s > 0)
    diff = r - s
    inl = meas & (np.abs(diff) <= tau)
    out = np.zeros(len(r), api.SCORE)
    out["visible"] = vis.sum((1, 2))
    out["inlier"] = inl.sum((1, 2))
    out["occluded"] = (meas & (diff > tau)).sum((1, 2))
    out["violation"] = (meas & (diff < -tau)).sum((1, 2))
    out["missing"] = (vis & (s <= 0)).sum((1, 2))
    out["abs_err_sum"] = [int(np.abs(diff[i][inl[i]]).sum()) for i in range(len(r))]
    return out


def assert_scores_equal(got, want):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:10], got[f][:10], want[f][:10])
    assert np.array_equal(got["visible"].astype(np.int64),
                          got["inlier"].astype(np.int64) + got["occluded"] + got["violation"] + got["missing"])


def assert_records_repeat(got, want):
    """got[i] == want[i % len(want)] for every i, byte for byte: one comparison over the whole batch."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)[np.arange(len(got)) % len(want)]
    bad = np.flatnonzero((g != w).any(1))
    assert len(bad) == 0, (len(bad), bad[:10], got[bad[:3]], want[bad[:3] % len(want)])


@functools.lru_cache(maxsize=None)
def launch_split_case():
    """A batch too large for one launch over its boxes (grid.y is limited): 8 poses of a 12-triangle box on a 48 x 32 frame -- two row blocks
    of 16, a width that is no multiple of 64 -- repeated to 32768 + 5 hypotheses by the caller.  The renders reach all four frame borders and
    cross the row-block boundary.  Returns a dict the tests share and leave as it is; tests/test_contour_host.py pins what it holds."""
    import oracle_lib as O
    from contour_ref import contour_ref, edge_distance_ref
    w, h, tau, jump, radius = 48, 32, 4, 10, 1
    v = np.array([[x, y, z] for x in (-60, 60) for y in (-45, 45) for z in (-30, 30)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.ascontiguousarray([[v[a], v[b], v[c]] for i, j, k, l in quads for a, b, c in ((i, j, k), (i, k, l))], np.float32)
    proj = api.compute_proj(np.array([60.0, 0, 23.5, 0, 60.0, 15.5, 0, 0, 1], np.float32), w, h)
    angles = [(0.3, 0.5, 0.1), (0.9, -0.4, 0.7), (-0.6, 0.2, 1.3), (1.4, 1.0, -0.3), (0.1, -1.1, 0.4), (-1.2, 0.6, 0.8), (0.7, 0.7, 0.7), (2.0, -0.2, -0.9)]
    shifts = [(0, 0, 400), (40, -30, 350), (-90, 60, 420), (120, 10, 380), (-20, 95, 300), (150, -80, 500), (-160, -10, 450), (10, 5, 260)]
    poses = np.stack([synth.pose_matrix(synth.euler_zyx(a), np.array(t, np.float32)) for a, t in zip(angles, shifts)])
    renders = O.render(tris, poses, w, h, proj)
    # the scene: what is in front among the first five renders with +-6 mm noise, a wall behind most of the rest, holes, a box in front
    rng = np.random.default_rng(5)
    front = np.where(renders[:5] > 0, renders[:5], 2**31 - 1).min(0)
    front[front == 2**31 - 1] = 0
    scene = front.astype(np.int64) + rng.integers(-6, 7, front.shape) * (front > 0)
    scene[(front == 0) & (rng.random(front.shape) < 0.6)] = 700
    scene[rng.random(front.shape) < 0.07] = 0
    scene[20:26, 30:40] = 150
    scene = scene.astype(np.int32)                                 # (every value fits uint16)
    dist = edge_distance_ref(scene, jump, radius)
    return dict(W=w, H=h, P=32768 + 5, tau=tau, jump=jump, radius=radius, tris=tris, proj=proj, poses=poses, renders=renders, scene=scene,
                dist=dist, scores=score_ref(renders, scene, tau), contours=contour_ref(renders, scene, tau, jump, dist))
