"""CPU reference of pr_score_cover / pr_select_cover_host: the cover rule in Python integers over boolean support masks, which come from
select_ref.support_ref on the oracle's renders (oracle_lib.render).  Also the straddler frame the cover tests share."""
import numpy as np

from pose_refine_amd import _lib, synth
from select_ref import shift, support_ref

NOT_IN_ORDER, EMPTY, ACCEPTED = _lib.COVER_NOT_IN_ORDER, _lib.COVER_EMPTY, _lib.COVER_ACCEPTED
REJ_THRESHOLD = _lib.COVER_REJECTED | _lib.COVER_REASON_THRESHOLD
REJ_CAP = _lib.COVER_REJECTED | _lib.COVER_REASON_CAP
NO_POSITION = 0xffffffff
KEEP_ALL = 0xffffffff

# the planted frame (select_ref.planted_frame) under (1, 2), min_new = 1 and rank_hypotheses' order: fresh of PLANTED_SELECTION in that order, claimed
PLANTED_FRESH = {5: ([11034, 20178, 10985], 42197), 10: ([11034, 20181, 10982], 42197)}


def supports_of(renders, scene, tau, roi=(0, 0, 0, 0)):
    """Per render the sorted flat indices (inside the ROI window when one is given) of its inlier pixels; renders may be any iterable."""
    scene = np.asarray(scene)
    if roi[2] > 0 and roi[3] > 0:
        x, y, w, h = roi
        scene = scene[y:y + h, x:x + w]
    return [np.flatnonzero(support_ref(r, scene, tau)) for r in renders], scene.size


def cover_ref(supports, n_pixels, order, new_num, new_den, min_new=1, max_keep=KEEP_ALL):
    """supports: per hypothesis the flat indices of its support (or a boolean mask).  Returns (selected list, COVER[P], COVER_FRAME record)."""
    sup = [np.flatnonzero(s) if np.asarray(s).dtype == np.bool_ else np.asarray(s, np.int64) for s in supports]
    P = len(sup)
    claimed = np.zeros(int(n_pixels), np.bool_)
    rec = np.zeros(P, _lib.COVER)
    rec["support"] = [len(s) for s in sup]
    rec["state"] = NOT_IN_ORDER
    rec["position"] = NO_POSITION
    sel, total = [], 0
    for i in (int(v) for v in order):
        size = int(rec["support"][i])
        if size == 0:
            rec["state"][i] = EMPTY
            continue
        if len(sel) >= int(max_keep):
            rec["state"][i] = REJ_CAP
            continue
        fresh = size - int(np.count_nonzero(claimed[sup[i]]))
        if fresh >= int(min_new) and fresh * int(new_den) >= int(new_num) * size:
            claimed[sup[i]] = True
            rec["fresh"][i], rec["state"][i], rec["position"][i] = fresh, ACCEPTED, len(sel)
            sel.append(i)
            total += fresh
        else:
            rec["state"][i] = REJ_THRESHOLD
    for i in range(P):
        if rec["state"][i] not in (ACCEPTED, EMPTY):
            rec["fresh"][i] = len(sup[i]) - int(np.count_nonzero(claimed[sup[i]]))
    frame = np.zeros(1, _lib.COVER_FRAME)
    frame["claimed"], frame["n_selected"] = total, len(sel)
    assert total == int(np.count_nonzero(claimed))
    return sel, rec, frame[0]


def masks_of(supports, n_pixels):
    """bool[P, n_pixels] from index lists (what api.select_cover_host packs into bit planes)."""
    m = np.zeros((len(supports), int(n_pixels)), np.bool_)
    for i, s in enumerate(supports):
        m[i, s] = True
    return m


def assert_cover_equal(got, want):
    """(cover, frame, selected) against cover_ref's (selected, cover, frame), byte for byte."""
    cov, frame, sel = got
    wsel, wcov, wframe = want
    assert cov.dtype == _lib.COVER and frame.dtype == _lib.COVER_FRAME
    bad = np.flatnonzero(cov != wcov)
    assert len(bad) == 0, (len(bad), bad[:8], cov[bad[:8]], wcov[bad[:8]])
    assert cov.tobytes() == wcov.tobytes() and frame.tobytes() == wframe.tobytes(), (frame, wframe)
    assert [int(i) for i in sel] == wsel


# ---- the straddler: two instances 120 mm apart in x and a third hypothesis halfway between them ------------------------------------------
STRADDLER_TAU = 10
STRADDLER_SUPPORT, STRADDLER_SHARED = 3519, (1684, 1835)      # the midpoint pose: its inlier pixels, and how many it shares with either instance


def straddler_frame(render, tris, W, H, proj):
    """(scene int32 (H, W), poses float32 (3, 4, 4)): the two instances, then the midpoint pose."""
    S = synth.scene_pose()
    poses = np.stack([S, S + shift(120, 0, 0), S + shift(60, 0, 0)]).astype(np.float32)
    r = render(tris, poses[:2], W, H, proj).astype(np.int64)
    scene = np.where(r > 0, r, 1 << 40).min(0)
    scene[scene == 1 << 40] = 0
    return scene.astype(np.int32), poses
