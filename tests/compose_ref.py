"""CPU reference of pr_compose_detections: the header's definitions in numpy over the oracle's renders (oracle_lib.render, bit-exact with the
HIP raster).  A key is (r << 32) | index in int64 -- r < 2^31, so it fits -- and the minimum over the hypotheses is the front depth with ties
to the lower index; the renders are taken one at a time, so an iterable of large frames works too."""
import numpy as np

from pose_refine_amd import api

NO_KEY = np.iinfo(np.int64).max
VISIBLE_FIELDS = ("owned", "owned_inlier", "owned_occluded", "owned_violation", "owned_missing")
FRAME_FIELDS = ("window", "measured", "covered", "explained", "in_front", "behind", "unmeasured", "reserved")


class Composite:
    """labels (H, W) uint16, depth (H, W) int32, visible VISIBLE[P], frame (one FRAME record), ties (H, W) int32: how many hypotheses attain
    the front depth at a pixel (0 where nothing is drawn)."""

    def __init__(self, labels, depth, visible, frame, ties):
        self.labels, self.depth, self.visible, self.frame, self.ties = labels, depth, visible, frame, ties


def compose_ref(renders, scene, tau, roi=(0, 0, 0, 0)):
    """renders: (P, rh, rw) int32 from oracle_lib.render, or any iterable of (rh, rw) renders (0 = nothing drawn; with a ROI, the window's
    pixels); scene: (H, W) int32 or uint16 frame."""
    scene = np.asarray(scene)
    H, W = scene.shape
    has_roi = roi[2] > 0 and roi[3] > 0
    x0, y0, rw, rh = roi if has_roi else (0, 0, W, H)
    key = np.full((rh, rw), NO_KEY, np.int64)
    ties = np.zeros((rh, rw), np.int32)
    P = 0
    for i, render in enumerate(renders):
        P = i + 1
        full = np.asarray(render)
        assert full.shape == (rh, rw), (full.shape, rh, rw)
        rows, cols = np.flatnonzero((full > 0).any(1)), np.flatnonzero((full > 0).any(0))
        if len(rows) == 0:
            continue
        box = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))      # only the render's own box changes (large frames)
        r = full[box].astype(np.int64)
        drawn = r > 0
        front = key[box] >> 32                                      # (2^31 - 1 where nothing is drawn yet: above every depth)
        ties[box] = np.where(drawn & (r < front), 1, ties[box] + (drawn & (r == front)))
        key[box] = np.minimum(key[box], np.where(drawn, (r << 32) | i, NO_KEY))
    covered = key != NO_KEY
    owner = (key & 0xffffffff).astype(np.int64)
    front = np.where(covered, key >> 32, 0)
    s = scene[y0:y0 + rh, x0:x0 + rw].astype(np.int64)
    diff = front - s
    meas = covered & (s > 0)
    classes = (meas & (np.abs(diff) <= tau), meas & (diff > tau), meas & (diff < -tau), covered & (s <= 0))      # inlier, occluded, violation, missing

    visible = np.zeros(P, api.VISIBLE)
    visible["owned"] = np.bincount(owner[covered], minlength=P)
    for f, m in zip(VISIBLE_FIELDS[1:], classes):
        visible[f] = np.bincount(owner[m], minlength=P)
    frame = np.zeros(1, api.FRAME)
    frame["window"], frame["measured"], frame["covered"] = rh * rw, int((s > 0).sum()), int(covered.sum())
    frame["explained"], frame["behind"], frame["in_front"], frame["unmeasured"] = (int(m.sum()) for m in classes)

    labels = np.full((H, W), api.COMPOSE_NONE, np.uint16)
    depth = np.zeros((H, W), np.int32)
    labels[y0:y0 + rh, x0:x0 + rw] = np.where(covered, owner, api.COMPOSE_NONE)
    depth[y0:y0 + rh, x0:x0 + rw] = front
    full_ties = np.zeros((H, W), np.int32)
    full_ties[y0:y0 + rh, x0:x0 + rw] = np.where(covered, ties, 0)
    return Composite(labels, depth, visible, frame[0], full_ties)


def check_invariants(c, scores=None):
    """What holds for every composite, of the reference or of the device."""
    v, f = c.visible, c.frame
    own = v["owned"].astype(np.int64)
    assert np.array_equal(own, sum(v[k].astype(np.int64) for k in VISIBLE_FIELDS[1:]))
    assert not v["reserved"].any() and f["reserved"] == 0
    assert int(f["covered"]) == int(f["explained"]) + int(f["in_front"]) + int(f["behind"]) + int(f["unmeasured"])
    assert int(own.sum()) == int(f["covered"]) and int(v["owned_inlier"].sum()) == int(f["explained"])
    assert int(v["owned_occluded"].sum()) == int(f["behind"]) and int(v["owned_violation"].sum()) == int(f["in_front"])
    assert int(v["owned_missing"].sum()) == int(f["unmeasured"])
    assert int(f["covered"]) <= int(f["window"]) and int(f["measured"]) <= int(f["window"])
    drawn = c.labels != api.COMPOSE_NONE
    assert np.array_equal(drawn, c.depth > 0) and int(drawn.sum()) == int(f["covered"])
    assert np.array_equal(np.bincount(c.labels[drawn].astype(np.int64), minlength=len(v)), own)
    if scores is not None:
        for a, b in zip(VISIBLE_FIELDS, ("visible", "inlier", "occluded", "violation", "missing")):
            assert (v[a] <= scores[b]).all(), (a, b)                # a hypothesis keeps a part of what it has on its own


def assert_composites_equal(got, want):
    for name in ("labels", "depth"):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, len(bad), bad[:10], g[tuple(bad[:10].T)], w[tuple(bad[:10].T)])
    for f in VISIBLE_FIELDS:
        assert np.array_equal(got.visible[f], want.visible[f]), (f, np.flatnonzero(got.visible[f] != want.visible[f])[:10], got.visible[f][:10], want.visible[f][:10])
    assert not got.visible["reserved"].any()
    for f in FRAME_FIELDS:
        assert int(got.frame[f]) == int(want.frame[f]), (f, int(got.frame[f]), int(want.frame[f]))
